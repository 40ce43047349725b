"""GPU input pipeline: the reference's per-image host work as three HIP kernels.

Reference (main process, one image at a time):
    ref/modules/loader.py:15-16   Image.open(path).convert('RGB').resize((256, 256)) ; ToTensor()
    ref/train.py:55               images = image_processor(images, return_tensors="pt").to(device_id)
Everything after the file read runs on the GPU and is bit-identical to Pillow at every uint8 stage: JPEG reconstruction
(`csrc/jpeg.hip`: dequantisation, inverse DCT, chroma upsampling, colour transform; only the serial Huffman decoding stays on the
host, in C++ threads, `csrc/jpeg_host.cpp`), both Pillow resizes, the float conversion, the processor's rescale (twice, as the
reference effectively does) and normalisation (`csrc/image_pre.hip`).  Entry points:

    GpuImageProcessor()(images)                 drop-in for `image_processor(images, return_tensors="pt")`: `images` is the
                                                DataLoader's [B, 3, 256, 256] float batch in [0, 1] (or a list of such CHW tensors)
    GpuImageProcessor().from_decoded(arrays)    list of decoded HWC uint8 RGB images of ANY size (numpy / PIL.Image / tensor):
                                                replaces loader.py:15-16 as well (use `DatasetLoader(decode_only=True)`)
    GpuImageProcessor().from_jpeg(files)        list of JPEG files (paths or bytes): replaces `Image.open(path).convert('RGB')` too.
                                                Baseline and progressive Huffman files; a CMYK, 12-bit or arithmetic-coded file
                                                raises NotImplementedError unless `other_formats="host"` is passed (then exactly
                                                those files are decoded with PIL and resized on the device like the rest)

Both return {"pixel_values": cuda float32 [B, 3, 224, 224]} -- what `MyModel.forward` takes.  No CPU fallback: without the HIP
library the call raises.

Train-time augmentation (`from_decoded` / `from_jpeg` only): `boxes=` ([n, 4] of top, left, h, w), `flips=` ([n] bool) or
`augment=RandomResizedCropFlip(...)` put a random resized crop and a horizontal flip where the reference loader resizes --
`im.crop(box).resize((256, 256))`, then `im.transpose(FLIP_LEFT_RIGHT)` -- inside the same three launches, bit for bit.
"""
import math

import numpy as np
import torch

from .. import ops

BILINEAR, BICUBIC = 2, 3


class BatchFeature(dict):
    """the `.to(device)`-able mapping `image_processor(...)` returns (ref/train.py:55 calls `.to(device_id)` on it)"""

    def to(self, device):
        return BatchFeature({k: v.to(device) for k, v in self.items()})

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


class RandomResizedCropFlip:
    """`torchvision.transforms.RandomResizedCrop.get_params` followed by `RandomHorizontalFlip`'s coin, draw for draw, as boxes and
    flags for `GpuImageProcessor.from_decoded / from_jpeg(augment=...)`.  All draws come from `generator` (torch's global CPU
    generator when None), image by image: the box of image 0, its flip, the box of image 1, ... so a seed fixes the batch."""

    def __init__(self, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip_p=0.5, generator=None):
        for name, v in (("scale", scale), ("ratio", ratio)):
            if len(v) != 2 or not all(math.isfinite(x) for x in v) or not 0 < v[0] <= v[1]:
                raise ValueError(f"{name} must be (min, max) with 0 < min <= max, got {v!r}")
        if not 0 <= flip_p <= 1:
            raise ValueError(f"flip_p must lie in [0, 1], got {flip_p!r}")
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        self.flip_p, self.generator = float(flip_p), generator

    def _box(self, height, width):
        g = self.generator
        area = height * width
        log_ratio = torch.log(torch.tensor(self.ratio))
        for _ in range(10):
            target_area = area * torch.empty(1).uniform_(self.scale[0], self.scale[1], generator=g).item()
            aspect = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=g)).item()
            w = int(round(math.sqrt(target_area * aspect)))
            h = int(round(math.sqrt(target_area / aspect)))
            if 0 < w <= width and 0 < h <= height:
                top = torch.randint(0, height - h + 1, size=(1,), generator=g).item()
                left = torch.randint(0, width - w + 1, size=(1,), generator=g).item()
                return top, left, h, w
        in_ratio = float(width) / float(height)  # no try fitted: the central crop
        if in_ratio < min(self.ratio):
            w = width
            h = int(round(w / min(self.ratio)))
        elif in_ratio > max(self.ratio):
            h = height
            w = int(round(h * max(self.ratio)))
        else:
            w, h = width, height
        return (height - h) // 2, (width - w) // 2, h, w

    def sample(self, sizes):
        """sizes: list of (height, width) -> (boxes int64 [n, 4] of top, left, h, w; flips bool [n]), CPU tensors"""
        boxes = torch.zeros(len(sizes), 4, dtype=torch.int64)
        flips = torch.zeros(len(sizes), dtype=torch.bool)
        for i, (height, width) in enumerate(sizes):
            boxes[i] = torch.tensor(self._box(int(height), int(width)))
            flips[i] = bool(torch.rand(1, generator=self.generator) < self.flip_p)
        return boxes, flips


def resolve_augment(sizes, boxes=None, flips=None, augment=None):
    """Host-side check of the augmentation arguments against the batch's `sizes` (list of (height, width)), before anything is
    enqueued.  Returns (None, None) when none is given -- the un-augmented call -- else (boxes int64 numpy [n, 4], flips bool numpy
    [n]), a missing one filled with the whole image / no flip.  A violation raises ValueError naming the image."""
    if augment is not None:
        if boxes is not None or flips is not None:
            raise ValueError("augment= draws the boxes and flips itself: pass either augment or boxes / flips")
        boxes, flips = augment.sample([(int(h), int(w)) for h, w in sizes])
    if boxes is None and flips is None:
        return None, None
    n = len(sizes)
    if boxes is None:
        b = np.array([(0, 0, h, w) for h, w in sizes], np.int64).reshape(n, 4)
    else:
        b = boxes.detach().cpu().numpy() if isinstance(boxes, torch.Tensor) else np.asarray(boxes)
        if b.shape != (n, 4):
            raise ValueError(f"boxes must be [{n}, 4] rows of (top, left, h, w), got shape {tuple(b.shape)}")
        if b.dtype.kind not in "iu":
            raise ValueError(f"boxes must be integers, got {b.dtype}")
        b = b.astype(np.int64)
    if flips is None:
        f = np.zeros(n, bool)
    else:
        f = flips.detach().cpu().numpy() if isinstance(flips, torch.Tensor) else np.asarray(flips)
        if f.shape != (n,):
            raise ValueError(f"flips must be [{n}] booleans, got shape {tuple(f.shape)}")
        if f.dtype != bool:
            raise ValueError(f"flips must be booleans, got {f.dtype}")
    sz = np.asarray([(int(h), int(w)) for h, w in sizes], np.int64).reshape(n, 2)
    empty = (b[:, 2] < 1) | (b[:, 3] < 1)
    outside = (b[:, 0] < 0) | (b[:, 1] < 0) | (b[:, 0] + b[:, 2] > sz[:, 0]) | (b[:, 1] + b[:, 3] > sz[:, 1])
    if (empty | outside).any():
        i = int(np.flatnonzero(empty | outside)[0])
        box = tuple(int(v) for v in b[i])
        if empty[i]:
            raise ValueError(f"image {i}: empty crop box (top, left, h, w) = {box}")
        raise ValueError(f"image {i}: crop box (top, left, h, w) = {box} leaves the {sz[i, 0]} x {sz[i, 1]} image")
    return b, f


class GpuImageProcessor:
    def __init__(self, size=224, resample=BILINEAR, rescale_factor=1 / 255, image_mean=(0.5, 0.5, 0.5), image_std=(0.5, 0.5, 0.5),
                 loader_size=256, loader_resample=BICUBIC, device="cuda"):
        """defaults = `ViTImageProcessor()` (HF/vitproc:20-27) behind the reference loader's 256x256 BICUBIC resize"""
        if isinstance(size, dict):
            if size["height"] != size["width"]:
                raise NotImplementedError("square outputs only")
            size = size["height"]
        self.size, self.resample = int(size), int(resample)
        self.mean, self.std = tuple(float(m) for m in image_mean), tuple(float(s) for s in image_std)
        self.loader_size, self.loader_resample = int(loader_size), int(loader_resample)
        # the processor turns [0,1] floats back into uint8 for Pillow, scales the result by 1/255 and THEN applies do_rescale
        self.rescale = (1.0 / 255.0) * float(rescale_factor)
        self.device = torch.device(device)

    # `preprocessor_config.json` of the hub checkpoints the reference's CLI accepts (ref/modules/config.py:6-7), restated from
    # the public model cards: ViTImageProcessor, 256x256, BICUBIC, ImageNet mean / std.  Used when the NAME is given and no
    # local directory exists (no hub access here); anything else must be a local directory or explicit keyword arguments.
    KNOWN = {name: dict(size=256, resample=BICUBIC, rescale_factor=1 / 255, image_mean=(0.485, 0.456, 0.406),
                        image_std=(0.229, 0.224, 0.225))
             for name in ("microsoft/swinv2-tiny-patch4-window8-256", "microsoft/swinv2-small-patch4-window8-256",
                          "microsoft/swinv2-base-patch4-window8-256", "microsoft/swinv2-base-patch4-window16-256")}

    @classmethod
    def from_pretrained(cls, path=None, **kw):
        """`AutoImageProcessor.from_pretrained(args.image_model_name)` (ref/train.py:39): a local directory with
        `preprocessor_config.json`, or one of the KNOWN hub names.  Anything else raises OSError like the reference does
        offline -- it never falls back to bare ViTImageProcessor defaults (a silent 224 / bilinear / 0.5-mean pipeline for a
        256 / bicubic / ImageNet checkpoint).  Explicit keyword arguments alone (path=None) build a processor directly."""
        import json
        import os
        keys = ("size", "resample", "rescale_factor", "image_mean", "image_std")
        if path is None:
            if not kw:
                raise OSError("GpuImageProcessor.from_pretrained needs a local directory, a known checkpoint name or explicit settings")
            return cls(**kw)
        cfg_file = os.path.join(path, "preprocessor_config.json") if os.path.isdir(path) else None
        if cfg_file and os.path.exists(cfg_file):
            with open(cfg_file) as f:
                cfg = json.load(f)
            for flag in ("do_resize", "do_rescale", "do_normalize"):
                if cfg.get(flag, True) is False:
                    raise NotImplementedError(f"preprocessor_config.json sets {flag}=false: outside the reference's pipeline")
            return cls(**{**{k: cfg[k] for k in keys if k in cfg}, **kw})
        if path in cls.KNOWN:
            return cls(**{**cls.KNOWN[path], **kw})
        raise OSError(f"Can't load image processor for '{path}': not a local directory containing preprocessor_config.json and not "
                      f"one of {sorted(cls.KNOWN)} (this build has no hub access).")

    def _out(self, n):
        return torch.empty(n, 3, self.size, self.size, dtype=torch.float32, device=self.device)

    def __call__(self, images, return_tensors="pt"):
        if return_tensors != "pt":
            raise ValueError("return_tensors must be 'pt'")
        if isinstance(images, (list, tuple)):
            images = torch.stack([torch.as_tensor(i) for i in images])
        if images.dim() == 3:
            images = images.unsqueeze(0)
        if images.dtype == torch.uint8:
            raise TypeError("uint8 images: use from_decoded() (HWC, any size)")
        B, C, H, W = images.shape
        if C != 3 or H != W:
            raise ValueError("expected [B, 3, S, S] float images in [0, 1] (the reference DataLoader's batches)")
        # [0,1] floats -> the uint8 image Pillow sees (HF to_pil_image: x * 255 -> uint8, truncating; exact for k / 255)
        u8 = (images.to(self.device, non_blocking=True) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        pv = self._out(B)
        ops.image_preprocess(u8, None, B, H, W, pv, mid=H, out=self.size, filter_a=0, filter_b=self.resample, rescale=self.rescale,
                             mean=self.mean, std=self.std)
        return BatchFeature(pixel_values=pv)

    def _augmented(self, pv, boxes, flips, sampled):
        out = BatchFeature(pixel_values=pv)
        if sampled:  # what was drawn, for logging and replay through boxes= / flips=
            out["crop_boxes"], out["flips"] = torch.from_numpy(boxes.copy()), torch.from_numpy(flips.copy())
        return out

    def from_decoded(self, images, boxes=None, flips=None, augment=None):
        """list of decoded RGB images (HWC uint8 numpy arrays, PIL images or tensors) of any size.  boxes ([n, 4] ints: top, left,
        h, w) / flips ([n] bools), or augment (a RandomResizedCropFlip that draws both; the result then also carries `crop_boxes`
        and `flips`): image i is cropped to its box before the loader's resize and mirrored left-right after it."""
        arrs = [np.asarray(im.convert("RGB") if hasattr(im, "convert") else im, dtype=np.uint8) for im in images]
        for a in arrs:
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("expected HWC RGB uint8 images")
        n = len(arrs)
        boxes, flips = resolve_augment([a.shape[:2] for a in arrs], boxes, flips, augment)
        sizes = [a.shape[0] * a.shape[1] * 3 for a in arrs]
        offs = np.concatenate([[0], np.cumsum([(s + 15) // 16 * 16 for s in sizes])]).astype(np.int64)
        total = int(offs[-1])
        # two pinned staging buffers, grown on demand and alternated: the async H2D copy of batch i may still be reading one
        # while batch i+1 is packed into the other (pinning per call costs more than the whole pipeline)
        self._flip = 1 - getattr(self, "_flip", 0)
        stage = getattr(self, "_stage", None) or [None, None]
        if stage[self._flip] is None or stage[self._flip].numel() < total:
            stage[self._flip] = torch.empty(max(total, 1), dtype=torch.uint8).pin_memory()
        self._stage = stage
        ev = getattr(self, "_stage_ev", None) or [None, None]
        if ev[self._flip] is not None:
            ev[self._flip].synchronize()  # the copy that last used this buffer has finished
        host = stage[self._flip][:total]
        hb = host.numpy()
        desc = np.zeros((n, 2), np.int64)
        for i, a in enumerate(arrs):
            hb[offs[i]:offs[i] + sizes[i]] = a.reshape(-1)
            desc[i, 0] = offs[i]
            desc[i, 1] = a.shape[0] | (a.shape[1] << 32)  # {int height, width} little-endian
        src = host.to(self.device, non_blocking=True)
        ev[self._flip] = torch.cuda.Event()
        ev[self._flip].record()
        self._stage_ev = ev
        pv = self._out(n)
        kw = dict(mid=self.loader_size, out=self.size, filter_a=self.loader_resample, filter_b=self.resample, rescale=self.rescale,
                  mean=self.mean, std=self.std)
        if boxes is not None:  # the crops are read in place: the whole images are staged as above, the descriptor points into them
            cd = ops.image_crop_desc(offs[:n], [a.shape[:2] for a in arrs], boxes, flips)
            ops.image_preprocess_crop(src, torch.from_numpy(cd).to(self.device), n, int(boxes[:, 2].max()), int(boxes[:, 3].max()), pv, **kw)
            return self._augmented(pv, boxes, flips, augment is not None)
        dd = torch.from_numpy(desc).to(self.device)
        ops.image_preprocess(src, dd, n, max(a.shape[0] for a in arrs), max(a.shape[1] for a in arrs), pv, **kw)
        return BatchFeature(pixel_values=pv)

    def from_jpeg(self, files, n_threads=None, other_formats="raise", boxes=None, flips=None, augment=None):
        """list of image files (paths, bytes or binary file objects) -> pixel_values; `Image.open(f).convert('RGB')` + from_decoded.
        Files the device decoder does not take (CMYK / 12-bit / arithmetic-coded JPEG, PNG, ...): other_formats="raise" (default)
        raises NotImplementedError naming them; other_formats="host" -- an explicit request, never a silent fallback -- decodes
        exactly those files with PIL on the host and sends them through the same device resize (`from_decoded`).
        boxes / flips / augment: as in `from_decoded`, against the sizes in the files' headers; the whole image is decoded on the
        device and the crop is read out of it in place."""
        if other_formats not in ("raise", "host"):
            raise ValueError("other_formats must be 'raise' or 'host'")
        datas = []
        for f in files:
            if isinstance(f, (bytes, bytearray, memoryview)):
                datas.append(bytes(f))
            elif hasattr(f, "read"):
                datas.append(f.read())
            else:
                with open(f, "rb") as fh:
                    datas.append(fh.read())
        if n_threads is None:
            import os
            n_threads = min(16, os.cpu_count() or 1)
        n = len(datas)
        aug = boxes is not None or flips is not None or augment is not None
        dev_idx, host_idx = list(range(n)), []
        sizes = [None] * n  # (height, width) from the headers: read for the host route, and to check the boxes before any launch
        if other_formats == "host":
            dev_idx = []
            for i, d in enumerate(datas):
                try:
                    info = ops.jpeg_read_info(d)
                    ok, sizes[i] = bool(info.supported), (info.height, info.width)
                except ValueError:  # not a JPEG stream at all
                    ok = False
                (dev_idx if ok else host_idx).append(i)
        host_imgs = []
        if host_idx:
            import io
            from PIL import Image
            host_imgs = [Image.open(io.BytesIO(datas[i])) for i in host_idx]
            for i, im in zip(host_idx, host_imgs):
                sizes[i] = (im.height, im.width)

        def check(dev_sizes=()):  # every size is known: check the boxes (or draw them), before anything is enqueued
            nonlocal boxes, flips
            for i, hw in zip(dev_idx, dev_sizes):
                sizes[i] = hw
            boxes, flips = resolve_augment(sizes, boxes, flips, augment)

        # other_formats="host" has read every header above; otherwise the decoder reads them, and hands the sizes over before it
        # allocates or enqueues anything
        hook = check if aug and dev_idx and other_formats == "raise" else None
        if aug and hook is None:
            check()
        pv = self._out(n)
        if dev_idx:
            sub = [datas[i] for i in dev_idx]
            rgb, desc, items = ops.jpeg_decode_pipelined(sub, self.device, n_threads, on_headers=hook)
            out = pv if not host_idx else self._out(len(sub))
            kw = dict(mid=self.loader_size, out=self.size, filter_a=self.loader_resample, filter_b=self.resample, rescale=self.rescale,
                      mean=self.mean, std=self.std)
            if aug:
                cd = ops.image_crop_desc([it.rgb_off for it in items], [(it.info.height, it.info.width) for it in items], boxes[dev_idx],
                                         flips[dev_idx])
                ops.image_preprocess_crop(rgb, torch.from_numpy(cd).to(self.device), len(sub), int(boxes[dev_idx, 2].max()),
                                          int(boxes[dev_idx, 3].max()), out, **kw)
            else:
                ops.image_preprocess(rgb, desc, len(sub), max(it.info.height for it in items), max(it.info.width for it in items), out, **kw)
            if host_idx:
                pv[torch.tensor(dev_idx, device=self.device)] = out
        if host_idx:
            host_imgs = [im.convert("RGB") for im in host_imgs]
            dec = (self.from_decoded(host_imgs, boxes=boxes[host_idx], flips=flips[host_idx]) if aug else self.from_decoded(host_imgs))
            pv[torch.tensor(host_idx, device=self.device)] = dec["pixel_values"]
        if aug:
            return self._augmented(pv, boxes, flips, augment is not None)
        return BatchFeature(pixel_values=pv)
