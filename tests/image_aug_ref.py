"""Reference for the augmented image path (random resized crop + horizontal flip on the device), shared by
tests/test_image_aug_cpu.py and tests/test_image_aug_gpu.py.

Semantics: image `i` with box (top, left, h, w) and flag `flip` gives what

    im.crop((left, top, left + w, top + h)).resize((mid, mid), filter_a) ; .transpose(FLIP_LEFT_RIGHT) if flip ; processor

gives.  On the oracle (oracle/image_pre.py) that is a numpy slice, `resize_u8`, `[:, ::-1]` and `preprocess(filter_a=None)`.
Crop THEN resize: the taps are clamped at the crop's edges, which Pillow's `resize(box=...)` does not do.

`sample_boxes` restates torchvision's `RandomResizedCrop.get_params` + `RandomHorizontalFlip` draw for draw (torchvision itself is
not imported anywhere)."""
import math

import numpy as np
import torch

from oracle import image_pre as O

# (image height, image width, (top, left, h, w)): the crops of the GPU tests, at loader_size 24 unless a test says otherwise
CASES = {
    "down": (61, 83, (7, 9, 45, 60)),          # an interior crop reduced on both axes
    "up": (40, 50, (3, 11, 5, 28)),            # 5 x 28 enlarged to 24 (the width reduced a little, the height enlarged)
    "identity": (40, 50, (2, 13, 30, 24)),     # the crop's width equals mid: Pillow skips the horizontal pass
    "odd_left": (33, 47, (4, 7, 20, 31)),      # byte offset (4 * 47 + 7) * 3 = 585: not a multiple of 4
    "rows15": (40, 37, (5, 3, 15, 30)),        # the 16-row block edge of the horizontal pass
    "rows16": (40, 37, (5, 3, 16, 30)),
    "rows17": (40, 37, (5, 3, 17, 30)),
    "single": (9, 11, (8, 10, 1, 1)),          # the last pixel of its image
    "wide": (4, 9000, (0, 4450, 4, 100)),      # an image the un-cropped path refuses (weight table beyond the LDS), a crop that fits
}
FULL = (480, 640)  # the one full-size case, at the default 256 / 224, boxes from the sampler (seed FULL_SEED)
FULL_SEED = 2024


def synth(h, w, seed):
    """an image with structure at every scale and full-range noise, so that a tap outside the crop changes the result"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([127 + 100 * np.sin(xx / 3.0) * np.cos(yy / 5.0), 255.0 * xx / max(w - 1, 1) + 0 * yy, 255.0 * yy / max(h - 1, 1) + 0 * xx], axis=2)
    return np.clip(a + rng.integers(-60, 61, a.shape), 0, 255).astype(np.uint8)


def mid_image(img, box, flip, mid, filter_a):
    """the loader's mid x mid uint8 image of the augmented chain"""
    top, left, h, w = (int(v) for v in box)
    m = O.resize_u8(img[top:top + h, left:left + w], mid, mid, filter_a)
    return np.ascontiguousarray(m[:, ::-1]) if flip else m


def reference(img, box, flip, mid=256, out=224, filter_a=O.BICUBIC, filter_b=O.BILINEAR):
    """-> (pixel_values CHW float32, the out x out uint8 image behind it), default mean / std / rescale"""
    return O.preprocess(mid_image(img, box, flip, mid, filter_a), mid=mid, out=out, filter_a=None, filter_b=filter_b)


def sample_boxes(sizes, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip_p=0.5, generator=None):
    """torchvision.transforms.RandomResizedCrop.get_params(img, scale, ratio), then `torch.rand(1) < p` of RandomHorizontalFlip,
    image by image; sizes: list of (height, width) -> (list of (top, left, h, w), list of bool)"""
    boxes, flips = [], []
    for height, width in sizes:
        area = height * width
        log_ratio = torch.log(torch.tensor(ratio))
        box = None
        for _ in range(10):
            target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
            aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=generator)).item()
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if 0 < w <= width and 0 < h <= height:
                i = torch.randint(0, height - h + 1, size=(1,), generator=generator).item()
                j = torch.randint(0, width - w + 1, size=(1,), generator=generator).item()
                box = (i, j, h, w)
                break
        if box is None:
            in_ratio = float(width) / float(height)
            if in_ratio < min(ratio):
                w = width
                h = int(round(w / min(ratio)))
            elif in_ratio > max(ratio):
                h = height
                w = int(round(h * max(ratio)))
            else:
                w = width
                h = height
            box = ((height - h) // 2, (width - w) // 2, h, w)
        boxes.append(box)
        flips.append(bool(torch.rand(1, generator=generator) < flip_p))
    return boxes, flips
