"""Several captions per image, the parts that need no device: COCODatasetLoader(captions_per_image=n), flatten_captions /
group_targets, the shape checks of MyModel.forward on [B, n, Lt] labels, the new C entry point, and the arithmetic facts the GPU
tests of tests/test_multi_caption_attn_gpu.py lean on (their fixtures are bf16 numbers at the cross-attention shapes, per
caption as well as per image)."""
import json
import os
import types

import pytest
import torch

from tests import exact_ref as R
from tests.helpers import load_golden

ANNOTATIONS = {
    "images": [{"id": 7, "file_name": "a.jpg"}, {"id": 3, "file_name": "b.jpg"}, {"id": 9, "file_name": "c.jpg"}],
    # file order, image ids interleaved: image 7 has three captions, image 3 five, image 9 one
    "annotations": [{"image_id": 7, "caption": "a0"}, {"image_id": 3, "caption": "b0"}, {"image_id": 7, "caption": "a1"},
                    {"image_id": 9, "caption": "c0"}, {"image_id": 3, "caption": "b1"}, {"image_id": 3, "caption": "b2"},
                    {"image_id": 7, "caption": "a2"}, {"image_id": 3, "caption": "b3"}, {"image_id": 3, "caption": "b4"}],
}


@pytest.fixture()
def coco_dir(tmp_path):
    os.makedirs(tmp_path / "annotations")
    with open(tmp_path / "annotations" / "captions_train2017.json", "w") as f:
        json.dump(ANNOTATIONS, f)
    return str(tmp_path)


def test_loader_default_is_the_first_caption_as_a_string(coco_dir):
    from klab_multimodalmodel_amd.modules.loader import COCO_PROMPT, COCODatasetLoader
    d = COCODatasetLoader(coco_dir, "train")
    assert d.captions_per_image == 1
    assert d.tgt_texts == ["a0", "b0", "c0"] and d.src_texts == [COCO_PROMPT] * 3
    assert [os.path.basename(p) for p in d.images] == ["a.jpg", "b.jpg", "c.jpg"]
    assert COCODatasetLoader(coco_dir, "train", captions_per_image=1).tgt_texts == d.tgt_texts


def test_loader_n_captions_in_file_order_filled_up_with_the_empty_marker(coco_dir):
    from klab_multimodalmodel_amd.modules.loader import NO_CAPTION, COCODatasetLoader
    d = COCODatasetLoader(coco_dir, "train", captions_per_image=4)
    assert d.tgt_texts == [["a0", "a1", "a2", NO_CAPTION], ["b0", "b1", "b2", "b3"], ["c0", NO_CAPTION, NO_CAPTION, NO_CAPTION]]
    assert COCODatasetLoader(coco_dir, "train", captions_per_image=2).tgt_texts == [["a0", "a1"], ["b0", "b1"], ["c0", NO_CAPTION]]
    for bad in (0, -1):
        with pytest.raises(ValueError, match="captions_per_image"):
            COCODatasetLoader(coco_dir, "train", captions_per_image=bad)


def test_flatten_captions_is_image_major_from_either_collate():
    from klab_multimodalmodel_amd.modules.loader import flatten_captions
    items = [["a0", "a1", "a2"], ["b0", "b1", "b2"]]  # [B][n]
    assert flatten_captions(items) == ["a0", "a1", "a2", "b0", "b1", "b2"]
    transposed = torch.utils.data.default_collate(items)  # torch's default collate of a batch of lists: [n][B]
    assert [list(r) for r in transposed] == [["a0", "b0"], ["a1", "b1"], ["a2", "b2"]]
    assert flatten_captions(transposed, image_major=False) == flatten_captions(items)
    with pytest.raises(ValueError, match="same number of captions"):
        flatten_captions([["a0", "a1"], ["b0"]])


def test_group_targets_shapes_and_minus_100_on_the_padded_captions():
    from klab_multimodalmodel_amd.modules.loader import NO_CAPTION, group_targets
    B, n, Lt = 2, 3, 4
    texts = ["a0", "a1", NO_CAPTION, "b0", NO_CAPTION, NO_CAPTION]
    ids = torch.arange(1, B * n * Lt + 1).view(B * n, Lt)
    enc = {"input_ids": ids, "attention_mask": torch.ones_like(ids)}
    out = group_targets(enc, texts, n)
    assert out["input_ids"].shape == (B, n, Lt) and out["attention_mask"].shape == (B, n, Lt)
    assert out["input_ids"].dtype == torch.int64
    empty = torch.tensor([[False, False, True], [False, True, True]])
    assert bool((out["input_ids"][empty] == -100).all())
    assert torch.equal(out["input_ids"][~empty], ids.view(B, n, Lt)[~empty])  # image-major: row b*n + j is caption j of image b
    assert torch.equal(ids, torch.arange(1, B * n * Lt + 1).view(B * n, Lt))  # the tokenizer's output is left alone
    assert torch.equal(out["attention_mask"], torch.ones(B, n, Lt, dtype=torch.int64))
    # n = 1: [B, 1, Lt], nothing masked
    one = group_targets({"input_ids": ids}, ["x"] * (B * n), 1)
    assert one["input_ids"].shape == (B * n, 1, Lt) and torch.equal(one["input_ids"].view(B * n, Lt), ids)
    with pytest.raises(ValueError, match="no multiple"):
        group_targets(enc, texts[:5], n)
    with pytest.raises(ValueError, match=r"\[B\*n, Lt\]"):
        group_targets({"input_ids": ids[:4]}, texts, n)


def _model():
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_golden("tiny_a")
    sw, t5 = SwinConfig.from_dict(g["meta"]["swin_config"]), T5Config.from_dict(g["meta"]["t5_config"])
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    return MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], g["sds"]["main"]), dtype=torch.float32), g


def test_forward_shape_checks_name_the_3d_shape():
    """the checks run before anything touches a device: CPU tensors are enough to reach them"""
    m, g = _model()
    inp = g["inputs"]
    B, Lt, n = inp["tgt_ids"].shape[0], inp["tgt_ids"].shape[1], 2
    images, src = {"pixel_values": inp["pixel_values"]}, {"input_ids": inp["src_ids"]}
    tgt = inp["tgt_ids"][:, None, :].repeat(1, n, 1)
    for w in (torch.ones(B, Lt), torch.ones(B * n, Lt), torch.ones(B, n, Lt + 1), torch.ones(B, n, Lt, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"\[B, n, Lt\] = \(%d, %d, %d\)" % (B, n, Lt)):
            m(images, src, {"input_ids": tgt, "loss_weights": w})
        assert m._loss_weights_next is None
    # the 2-D message is what it was
    with pytest.raises(ValueError, match=r"float tensor \(%d, %d\)" % (B, Lt)):
        m(images, src, {"input_ids": inp["tgt_ids"], "loss_weights": torch.ones(B, n, Lt)})
    with pytest.raises(ValueError, match=r"\[B, n, Lt\] is on meta"):
        m(images, src, {"input_ids": tgt, "loss_weights": torch.ones(B, n, Lt, device="meta")})
    # labels of another rank, or of another number of images
    for bad in (inp["tgt_ids"][0], tgt[:, None], tgt[:1]):
        with pytest.raises(ValueError, match=r"\[B, Lt\] or \[B, n, Lt\]"):
            m(images, src, {"input_ids": bad})
    # a well-formed grouped call gets as far as the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(images, src, {"input_ids": tgt, "loss_weights": torch.ones(B, n, Lt)})


def test_entry_point_is_declared_and_workspace_grows_on_the_decoder_side_only():
    """klab_engine_set_captions is exported with its signature; the plan (host arithmetic only) at n = 1 is the plan without it,
    and n captions cost less than n times the batch"""
    from klab_multimodalmodel_amd import _lib as L
    assert L.SIGNATURES["klab_engine_set_captions"] == [L.vp, L.i32]
    m, _g = _model()
    eng = m._engine
    B, Ls, Lt = 4, 6, 9
    base = eng.workspace_bytes(B, Ls, Lt)
    assert eng.workspace_bytes(B, Ls, Lt, 1) == base
    three = eng.workspace_bytes(B, Ls, Lt, 3)
    assert base < three < eng.workspace_bytes(3 * B, Ls, Lt)
    assert eng.workspace_bytes(B, Ls, Lt) == base  # the default is n = 1 again, whatever the call before asked for
    # the query changes nothing: the C query without n sizes what the next bind would make, which a query for n = 3 leaves at 1
    plain = lambda: int(eng._lib.klab_engine_workspace_bytes(eng._h, B, Ls, Lt))
    assert plain() == base
    L.check(eng._lib.klab_engine_set_captions(eng._h, 3), "klab_engine_set_captions")
    assert plain() == three and eng.workspace_bytes(B, Ls, Lt, 1) == base and plain() == three
    L.check(eng._lib.klab_engine_set_captions(eng._h, 1), "klab_engine_set_captions")
    assert plain() == base
    with pytest.raises(ValueError):
        eng.workspace_bytes(B, Ls, Lt, 0)


# ---- the kernel-level GPU tests' fixtures ----------------------------------------------------------------------------------------
from tests.multi_caption_shapes import XATTN_B, XATTN_H, XATTN_SHAPES, caption_slices, xattn_kinds  # noqa: E402


@pytest.mark.parametrize("Lq,n,Lk,dk", XATTN_SHAPES, ids=lambda v: str(v))
def test_cross_attention_fixtures_are_bf16_exact_per_image_and_per_caption(Lq, n, Lk, dk):
    """what tests/test_multi_caption_attn_gpu.py compares bit for bit: every output of the B-batch, n*Lt-query problem is a bf16
    number, so is every output of each caption's own Lt-query problem, and d k / d v of the image are the sums of the captions'"""
    for kind, nk in xattn_kinds(dk):
        f = R.attn_fixture(kind, XATTN_B, XATTN_H, Lq, Lk, dk, False, nk)
        for name in ("q", "k", "v", "do", "ctx", "dS", "dq", "dk_", "dv"):
            assert R.bf16_exact(getattr(f, name)), (kind, name)
        assert float((f.softmax_fp64() - f.P).abs().max()) < 1e-50
        assert bool((f.dv != 0).any()) and bool((f.ctx != 0).any())
        sk, sv = torch.zeros_like(f.dk_), torch.zeros_like(f.dv)
        for sl in caption_slices(Lq, n):
            dS, Pm = f.dS[:, :, sl], f.Pm[:, :, sl]
            dk_j, dv_j = dS.transpose(-1, -2) @ f.q[:, :, sl], Pm.transpose(-1, -2) @ f.do[:, :, sl]
            assert R.bf16_exact(dk_j) and R.bf16_exact(dv_j), kind
            sk += dk_j
            sv += dv_j
        assert torch.equal(sk, f.dk_) and torch.equal(sv, f.dv)
