"""The augmented image path on the GPU (csrc/image_pre.hip through `klab_image_preprocess_crop`): a crop read in place and a
mirrored store, against the oracle chain of tests/image_aug_ref.py -- bit-exact on the uint8 stage, 1e-6 on pixel_values, as
tests/test_image_pre.py compares.  Small processors (loader_size 24 / 7 / 25) keep every case well under a second."""
import io

import numpy as np
import pytest
import torch

from oracle import image_pre as O
from tests import image_aug_ref as R

pytestmark = pytest.mark.gpu


def _proc(**kw):
    from klab_multimodalmodel_amd.modules.image_pipeline import GpuImageProcessor
    return GpuImageProcessor(**kw)


def _aug(**kw):
    from klab_multimodalmodel_amd.modules.image_pipeline import RandomResizedCropFlip
    return RandomResizedCropFlip(**kw)


@pytest.fixture(scope="module")
def small():
    return _proc(size=16, loader_size=24)


def _u8_of(pv):  # (holds for mean = std = 0.5 only: every processor here keeps the defaults)
    return np.rint((pv.astype(np.float64) * 0.5 + 0.5) * 255 * 255).astype(np.int64)


def _check(p, pv, img, box, flip, what):
    ref, u8 = R.reference(img, box, flip, mid=p.loader_size, out=p.size, filter_a=p.loader_resample, filter_b=p.resample)
    assert pv.shape == ref.shape, what
    assert np.array_equal(_u8_of(pv).transpose(1, 2, 0), u8.astype(np.int64)), what
    assert np.abs(pv - ref).max() <= 1e-6, what


def _run_case(p, name, flips=(False, True)):
    ih, iw, box = R.CASES[name]
    img = R.synth(ih, iw, len(name) + ih)
    for flip in flips:
        pv = p.from_decoded([img], boxes=[box], flips=[flip])["pixel_values"][0].cpu().numpy()
        _check(p, pv, img, box, flip, (name, flip))


@pytest.mark.parametrize("filt", [O.BICUBIC, O.BILINEAR])
def test_downscale_interior_crop(filt):
    _run_case(_proc(size=16, loader_size=24, loader_resample=filt), "down")


@pytest.mark.parametrize("name", ["up", "identity", "odd_left", "rows15", "rows16", "rows17"])
def test_crop_shapes(small, name):
    _run_case(small, name)


@pytest.mark.parametrize("size,mid", [(5, 7), (9, 25)])
def test_unpacked_vertical_pass(size, mid):
    """mid * 3 is no multiple of 4: the byte-wise vertical pass"""
    assert (mid * 3) % 4
    p = _proc(size=size, loader_size=mid)
    for name in ("down", "up", "rows17"):
        _run_case(p, name)


def test_single_pixel_at_the_end_of_the_buffer(small):
    """a 1 x 1 crop that is the last pixel of the last image: nothing behind it is read (its value alone decides the result)"""
    imgs = [R.synth(12, 16, 1), R.synth(9, 11, 2)]  # 9 * 11 * 3 = 297 bytes: the last pixel sits one byte short of the padded end
    box = R.CASES["single"][2]
    for flip in (False, True):
        out = small.from_decoded(imgs, boxes=[(0, 0, 12, 16), box], flips=[False, flip])["pixel_values"].cpu().numpy()
        _check(small, out[1], imgs[1], box, flip, flip)
        _check(small, out[0], imgs[0], (0, 0, 12, 16), False, flip)


def test_mixed_batch_entries_are_independent_and_repeatable(small):
    names = ["down", "up", "identity", "odd_left", "rows17", "single"]
    imgs = [R.synth(R.CASES[k][0], R.CASES[k][1], 40 + i) for i, k in enumerate(names)]
    boxes = [R.CASES[k][2] for k in names]
    flips = [True, False, True, True, False, True]
    a = small.from_decoded(imgs, boxes=boxes, flips=flips)["pixel_values"]
    b = small.from_decoded(imgs, boxes=np.array(boxes), flips=torch.tensor(flips))["pixel_values"]
    assert torch.equal(a, b)
    host = a.cpu().numpy()
    for i in range(len(imgs)):
        _check(small, host[i], imgs[i], boxes[i], flips[i], names[i])
        alone = small.from_decoded([imgs[i]], boxes=[boxes[i]], flips=[flips[i]])["pixel_values"]
        assert torch.equal(alone[0], a[i]), names[i]


def test_nothing_outside_the_box_leaks_in(small):
    ih, iw, box = R.CASES["down"]
    top, left, h, w = box
    a = R.synth(ih, iw, 3)
    b = 255 - R.synth(ih, iw, 4)
    b[top:top + h, left:left + w] = a[top:top + h, left:left + w]
    assert not np.array_equal(a, b)
    for flip in (False, True):
        out = small.from_decoded([a, b], boxes=[box, box], flips=[flip, flip])["pixel_values"]
        assert torch.equal(out[0], out[1]), flip


def test_neutral_arguments(small):
    sizes = [(31, 45), (24, 24), (50, 20)]
    imgs = [R.synth(h, w, 60 + i) for i, (h, w) in enumerate(sizes)]
    full = [(0, 0, h, w) for h, w in sizes]
    plain = small.from_decoded(imgs)
    assert set(plain) == {"pixel_values"}
    got = small.from_decoded(imgs, boxes=full, flips=[False] * 3)
    assert set(got) == {"pixel_values"} and torch.equal(got["pixel_values"], plain["pixel_values"])
    assert torch.equal(small.from_decoded(imgs, boxes=full)["pixel_values"], plain["pixel_values"])
    assert torch.equal(small.from_decoded(imgs, flips=[False] * 3)["pixel_values"], plain["pixel_values"])
    # flips only / boxes only
    fl = [True, False, True]
    out = small.from_decoded(imgs, flips=fl)["pixel_values"].cpu().numpy()
    for i in range(3):
        _check(small, out[i], imgs[i], full[i], fl[i], ("flips only", i))
    bx = [(3, 4, 20, 30), (0, 0, 24, 24), (10, 1, 40, 19)]
    out = small.from_decoded(imgs, boxes=bx)["pixel_values"].cpu().numpy()
    for i in range(3):
        _check(small, out[i], imgs[i], bx[i], False, ("boxes only", i))


def test_from_jpeg_equals_from_decoded_with_the_same_boxes():
    """on the files of tests/test_jpeg_gpu.py::test_from_jpeg_equals_from_decoded, the host route included"""
    from PIL import Image
    rng = np.random.default_rng(9)
    datas = []
    for (h, w, sub) in ((480, 640, 2), (333, 500, 2), (500, 375, 1), (640, 427, 0), (224, 224, 2), (97, 131, 2)):
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([127 + 100 * np.sin(xx / 17.0) * np.cos(yy / 23.0), 255.0 * xx / w + 0 * yy, 255.0 * yy / h + 0 * xx], axis=2)
        a = np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=88, subsampling=sub)
        datas.append(buf.getvalue())
    buf = io.BytesIO()
    Image.fromarray(rng.integers(0, 255, (300, 200), dtype=np.uint8), "L").save(buf, "JPEG", quality=70)
    datas.append(buf.getvalue())
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=85, progressive=True)
    datas.append(buf.getvalue())
    dec = [np.asarray(Image.open(io.BytesIO(d)).convert("RGB")) for d in datas]
    sizes = [d.shape[:2] for d in dec]
    boxes, flips = _aug(generator=torch.Generator().manual_seed(21)).sample(sizes)
    flips[::2] = True
    proc = _proc(size=32, loader_size=40)
    a = proc.from_jpeg(datas, boxes=boxes, flips=flips)
    b = proc.from_decoded(dec, boxes=boxes, flips=flips)
    assert set(a) == {"pixel_values"} and a["pixel_values"].shape == (len(datas), 3, 32, 32)
    assert torch.equal(a["pixel_values"], b["pixel_values"])
    host = a["pixel_values"].cpu().numpy()
    for i in (1, 5):
        _check(proc, host[i], dec[i], boxes[i].tolist(), bool(flips[i]), i)
    # the explicit host route hands ITS files' boxes and flips on, in batch order
    cmyk, png = io.BytesIO(), io.BytesIO()
    Image.fromarray(rng.integers(0, 255, (32, 32, 3), dtype=np.uint8)).convert("CMYK").save(cmyk, "JPEG")
    Image.fromarray(rng.integers(0, 255, (50, 70, 3), dtype=np.uint8)).save(png, "PNG")
    mixed = [datas[0], cmyk.getvalue(), datas[2], png.getvalue()]
    mdec = [np.asarray(Image.open(io.BytesIO(x)).convert("RGB")) for x in mixed]
    mb = [(100, 200, 300, 400), (5, 6, 20, 21), (0, 0, 500, 375), (49, 0, 1, 70)]
    mf = [False, True, True, False]
    c = proc.from_jpeg(mixed, other_formats="host", boxes=mb, flips=mf)["pixel_values"]
    d = proc.from_decoded(mdec, boxes=mb, flips=mf)["pixel_values"]
    assert torch.equal(c, d)
    with pytest.raises(ValueError, match="image 1"):  # checked against the header's size, before the decoder runs
        proc.from_jpeg(datas[:2], boxes=[(0, 0, 480, 640), (0, 0, 334, 500)])
    # augment= on files: the sizes come from the headers
    e = proc.from_jpeg(datas, augment=_aug(generator=torch.Generator().manual_seed(22)))
    rb, rf = R.sample_boxes(sizes, generator=torch.Generator().manual_seed(22))
    assert e["crop_boxes"].tolist() == [list(x) for x in rb] and e["flips"].tolist() == rf
    assert torch.equal(e["pixel_values"], proc.from_decoded(dec, boxes=rb, flips=rf)["pixel_values"])


def test_from_jpeg_on_every_decoder_case(small):
    """all files of tests/jpeg_cases.py (every sampling mode, grey, progressive, 1-pixel sizes) in one batch with drawn boxes"""
    from PIL import Image
    from tests.jpeg_cases import jpeg_cases
    datas = [d for _n, d in jpeg_cases()]
    dec = [np.asarray(Image.open(io.BytesIO(d)).convert("RGB")) for d in datas]
    a = small.from_jpeg(datas, augment=_aug(scale=(0.2, 1.0), generator=torch.Generator().manual_seed(31)))
    b = small.from_decoded(dec, boxes=a["crop_boxes"], flips=a["flips"])
    assert a["flips"].any() and not a["flips"].all()
    assert torch.equal(a["pixel_values"], b["pixel_values"])


def test_augment_is_replayable_and_seeded(small):
    sizes = [(61, 83), (40, 50), (33, 47), (10, 400), (24, 24)]
    imgs = [R.synth(h, w, 80 + i) for i, (h, w) in enumerate(sizes)]
    out = small.from_decoded(imgs, augment=_aug(generator=torch.Generator().manual_seed(5)))
    assert set(out) == {"pixel_values", "crop_boxes", "flips"}
    assert not out["crop_boxes"].is_cuda and out["crop_boxes"].dtype == torch.int64 and out["crop_boxes"].shape == (5, 4)
    assert not out["flips"].is_cuda and out["flips"].dtype == torch.bool and out["flips"].shape == (5,)
    rb, rf = R.sample_boxes(sizes, generator=torch.Generator().manual_seed(5))
    assert out["crop_boxes"].tolist() == [list(b) for b in rb] and out["flips"].tolist() == rf
    again = small.from_decoded(imgs, boxes=out["crop_boxes"], flips=out["flips"])
    assert torch.equal(again["pixel_values"], out["pixel_values"])
    same = small.from_decoded(imgs, augment=_aug(generator=torch.Generator().manual_seed(5)))
    assert torch.equal(same["pixel_values"], out["pixel_values"]) and torch.equal(same["crop_boxes"], out["crop_boxes"])
    other = small.from_decoded(imgs, augment=_aug(generator=torch.Generator().manual_seed(6)))
    assert not torch.equal(other["crop_boxes"], out["crop_boxes"])
    host = out["pixel_values"].cpu().numpy()
    for i in range(5):
        _check(small, host[i], imgs[i], rb[i], rf[i], i)
    with pytest.raises(ValueError, match="augment"):
        small.from_decoded(imgs, boxes=out["crop_boxes"], augment=_aug())


def test_full_size_batch_at_the_default_sizes():
    p = _proc()
    imgs = [R.synth(*R.FULL, 5 + i) for i in range(4)]
    out = p.from_decoded(imgs, augment=_aug(generator=torch.Generator().manual_seed(R.FULL_SEED)))
    rb, _rf = R.sample_boxes([R.FULL] * 4, generator=torch.Generator().manual_seed(R.FULL_SEED))
    assert out["crop_boxes"].tolist() == [list(b) for b in rb]
    flips = [True, False, False, True]  # fixed, so that both compared images are of one kind each
    pv = p.from_decoded(imgs, boxes=out["crop_boxes"], flips=flips)["pixel_values"]
    assert pv.shape == (4, 3, 224, 224)
    host = pv.cpu().numpy()
    for i in (0, 1):
        _check(p, host[i], imgs[i], rb[i], flips[i], i)


def test_an_image_too_wide_for_the_plain_path_is_taken_with_a_crop_that_fits():
    p = _proc()
    ih, iw, box = R.CASES["wide"]
    img = R.synth(ih, iw, 9)
    with pytest.raises(NotImplementedError):
        p.from_decoded([img])
    for flip in (False, True):
        pv = p.from_decoded([img], boxes=[box], flips=[flip])["pixel_values"][0].cpu().numpy()
        _check(p, pv, img, box, flip, flip)


def test_an_out_of_bounds_box_raises_before_any_launch(small, monkeypatch):
    from klab_multimodalmodel_amd import _lib
    lib, calls = _lib.load(), []
    for name in ("klab_image_preprocess", "klab_image_preprocess_crop", "klab_jpeg_decode_device", "klab_jpeg_entropy_decode_batch"):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: calls.append(_n) or 0)
    imgs = [R.synth(20, 30, 1), R.synth(20, 30, 2)]
    with pytest.raises(ValueError, match="image 1"):
        small.from_decoded(imgs, boxes=[(0, 0, 20, 30), (1, 0, 20, 30)])
    with pytest.raises(ValueError, match="image 0"):
        small.from_decoded(imgs, boxes=[(0, 0, 0, 30), (0, 0, 20, 30)])
    with pytest.raises(ValueError, match="flips"):
        small.from_decoded(imgs, flips=[True])
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(imgs[0]).save(buf, "JPEG")
    with pytest.raises(ValueError, match="image 0"):
        small.from_jpeg([buf.getvalue()], boxes=[(0, 0, 21, 30)])
    assert calls == []
