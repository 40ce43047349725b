"""Dataset surface of the reference (ref/modules/loader.py:8-88), host-side data prep only.

Same classes, same `__getitem__` results: image -> RGB -> 256x256 -> float CHW in [0,1]
(`torchvision.transforms.ToTensor` semantics, re-implemented with numpy because torchvision is not
required here); MSCOCO: first caption per image with the reference's fixed prompt (typo included);
RedCaps: word-level span masking, 15 % of the words + 1, `<extra_id_k>` sentinels
(ref/modules/loader.py:56-72).  The COCO annotation index is read directly from the JSON
(the reference's SilentCOCO, ref/modules/coco.py, is pycocotools with the prints removed).
"""
import json
import os

import numpy as np
import torch
from PIL import Image

COCO_PROMPT = 'What does th image describe ?'  # verbatim, ref/modules/loader.py:38
NO_CAPTION = ''  # fills an image's caption list up to captions_per_image; group_targets labels such a caption -100 throughout


def pil_to_tensor01(image):
    """ToTensor(): HWC uint8 -> CHW float32 / 255."""
    a = np.asarray(image, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(a.transpose(2, 0, 1).copy()).to(torch.float32).div_(255.0)


def span_mask(caption: str):
    """(src_text, tgt_text) of RedCapsDatasetLoader.__getitem__; consumes torch's global RNG exactly as the
    reference does (one `torch.randperm(len(words))`)."""
    for ch in '.,!?':
        caption = caption.replace(ch, ' ' + ch)
    words = caption.split()
    n_mask = int(len(words) * 0.15) + 1
    masked = set(torch.randperm(len(words))[:n_mask].tolist())
    tgt = ['<extra_id_0>']
    k = 0
    for i, w in enumerate(words):
        if i in masked:
            tgt.extend([w, f'<extra_id_{k + 1}>'])
            words[i] = f'<extra_id_{k}>'
            k += 1
    return ' '.join(words), ' '.join(tgt)


class DatasetLoader(torch.utils.data.Dataset):
    # decode_only (klab extension): __getitem__ returns the decoded HWC uint8 RGB image at its own size; the
    # 256x256 resize, ToTensor and the image processor then run on the GPU (`modules.image_pipeline.GpuImageProcessor
    # .from_decoded`, bit-identical to Pillow).  Batches of such items need `collate_decoded` (images stay a list).
    decode_only = False
    # file_bytes (klab extension): __getitem__ returns the JPEG file's bytes; decoding too then runs through
    # `GpuImageProcessor.from_jpeg` (host Huffman stage + device reconstruction, byte-identical to `Image.open().convert('RGB')`)
    file_bytes = False

    def __init__(self):
        self.images, self.tgt_texts, self.src_texts = [], [], []
        self.transform = pil_to_tensor01

    def _load_image(self, path):
        if self.file_bytes:
            with open(path, 'rb') as f:
                return f.read()
        if self.decode_only:
            return torch.from_numpy(np.asarray(Image.open(path).convert('RGB'), dtype=np.uint8).copy())
        return self.transform(Image.open(path).convert('RGB').resize((256, 256)))

    def __getitem__(self, idx):
        return self._load_image(self.images[idx]), self.src_texts[idx], self.tgt_texts[idx]

    def __len__(self):
        return len(self.images)


class COCODatasetLoader(DatasetLoader):
    # captions_per_image (klab extension; the reference keeps `loadAnns(...)[0]` only): 1 -- the item's target is the image's first
    # caption, a string, as in the reference; n > 1 -- a list of its first n captions in file order, filled up with NO_CAPTION
    # where the image has fewer.  MyModel.forward trains on all of them with one encoder pass per image (labels [B, n, Lt],
    # see flatten_captions / group_targets).
    def __init__(self, data_dir='/data/datatset/mscoco2017', phase='train', captions_per_image=1):
        super().__init__()
        n = int(captions_per_image)
        if n < 1:
            raise ValueError(f"`captions_per_image` has to be a positive integer, but is {captions_per_image}")
        self.captions_per_image = n
        with open(os.path.join(data_dir, 'annotations', f'captions_{phase}2017.json')) as f:
            ann = json.load(f)
        captions = {}
        for a in ann['annotations']:  # annotations per image, in file order (= coco.getAnnIds(image_id)); [0] is the reference's
            captions.setdefault(a['image_id'], []).append(a['caption'])
        img_dir = os.path.join(data_dir, f'{phase}2017')
        for info in ann['images']:
            self.images.append(os.path.join(img_dir, info['file_name']))
            self.src_texts.append(COCO_PROMPT)
            caps = captions[info['id']]
            self.tgt_texts.append(caps[0] if n == 1 else caps[:n] + [NO_CAPTION] * (n - len(caps[:n])))


class RedCapsDatasetLoader(DatasetLoader):
    def __init__(self, data_dir='/data/dataset/redcaps', phase='train'):
        super().__init__()
        anno_dir = os.path.join(data_dir, 'annotations')
        img_dir = os.path.join(data_dir, 'images')
        for name in os.listdir(anno_dir):
            with open(os.path.join(anno_dir, name)) as f:
                for ann in json.load(f)["annotations"]:
                    self.images.append(os.path.join(img_dir, ann["subreddit"], f"{ann['image_id']}.jpg"))
                    self.src_texts.append(ann['raw_caption'])

    def __getitem__(self, idx):
        src, tgt = span_mask(self.src_texts[idx])  # RNG is consumed before the image is opened, as in the reference
        return self._load_image(self.images[idx]), src, tgt


def collate_decoded(batch):
    """collate_fn for `decode_only` / `file_bytes` datasets: (list of HWC uint8 tensors or of JPEG byte strings, list of src texts,
    list of tgt texts)"""
    images, src, tgt = zip(*batch)
    return list(images), list(src), list(tgt)


def flatten_captions(tgt, image_major=True):
    """the B*n target strings of a batch of captions_per_image = n items in image-major order (image 0's n captions, then image
    1's, ...): what the tokenizer is called on.  image_major=True: tgt is [B][n], as collate_decoded (or any collate that keeps
    the items' lists) leaves it; False: [n][B], as torch's default collate transposes a batch of lists."""
    rows = [list(r) for r in tgt]
    if not rows or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("every image needs the same number of captions (COCODatasetLoader(captions_per_image=n) fills them up)")
    if not image_major:
        rows = [list(r) for r in zip(*rows)]
    return [c for r in rows for c in r]


def group_targets(encoding, texts, n):
    """target_encoding for MyModel.forward from a tokenizer output over the B*n strings of flatten_captions: every [B*n, Lt] tensor
    of `encoding` (input_ids, attention_mask, ...) viewed [B, n, Lt]; the labels of the captions that are NO_CAPTION set to -100
    throughout, so that they add nothing to the loss or the gradients."""
    n = int(n)
    if n < 1 or len(texts) % n:
        raise ValueError(f"{len(texts)} target strings are no multiple of n = {n} captions per image")
    out = {}
    for k in encoding.keys():
        v = encoding[k]
        if torch.is_tensor(v):
            if v.dim() != 2 or v.shape[0] != len(texts):
                raise ValueError(f"encoding[{k!r}] has to be [B*n, Lt] = [{len(texts)}, Lt], got {tuple(v.shape)}")
            v = v.reshape(len(texts) // n, n, v.shape[1])
        out[k] = v
    if "input_ids" not in out or not torch.is_tensor(out["input_ids"]):
        raise ValueError("encoding needs an `input_ids` tensor (tokenizer(..., return_tensors='pt'))")
    empty = torch.tensor([t == NO_CAPTION for t in texts], dtype=torch.bool, device=out["input_ids"].device)
    out["input_ids"] = out["input_ids"].masked_fill(empty.view(-1, n, 1), -100)
    return out


def get_dataloader(args, phase, rank):
    name = args.data_dir.lower()
    if 'mscoco' in name:
        dataset = COCODatasetLoader(args.data_dir, phase)
    elif 'redcaps' in name:
        dataset = RedCapsDatasetLoader(args.data_dir, phase)
    else:
        raise NotImplementedError
    # the reference sizes the sampler by the LOCAL device count and never calls set_epoch: kept
    sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=torch.cuda.device_count(), rank=rank,
                                                              shuffle=True, drop_last=True)
    gpu_pre = bool(getattr(args, 'gpu_preprocess', False))  # klab extension; the reference has no such flag (default off)
    dataset.decode_only = gpu_pre
    dataset.file_bytes = gpu_pre and bool(getattr(args, 'gpu_jpeg_decode', False))  # klab extension: batches carry file bytes
    return torch.utils.data.DataLoader(dataset, batch_size=args.batch_size, num_workers=os.cpu_count() // 4, pin_memory=not gpu_pre,
                                       sampler=sampler, collate_fn=collate_decoded if gpu_pre else None)
