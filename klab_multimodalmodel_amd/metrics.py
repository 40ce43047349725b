"""BLEU-1..4 and ROUGE-L of generated captions, computed on the device from integer sufficient statistics.

    stats = metrics.caption_stats(seq, refs_tensor)            # int32 [B, n, 16]: one launch, no host read
    scores = metrics.sentence_scores(stats)                    # fp64 [B, n, 5]: Bleu_1..4, ROUGE_L, still on the device
    cm = metrics.CaptionMetrics(cider=table)                   # a validation run: one device tensor of sums ...
    for images, source, refs_tensor in loader:
        cm.update(model.generate(pixels, src, max_length=20), refs_tensor)
    print(cm.compute())                                        # ... and one host read at the end

Inputs are scst.ciderd's: hyp int64 [B * n, L] as generate returns them (start token first, image-major) and refs int64 [B, R, Lr]
in label format (rows closed by EOS, an absent reference starts with a negative entry).  Units are a row's tokens through the first
EOS -- the EOS itself only when count_eos (off by default here: the COCO tools do not score the end of a caption) -- and an id < 0
or >= 0xFFFF ends the sequence.

The statistics of one hypothesis h against the present references r_j of its image (columns of the last axis):
    0..3   match_n, n = 1..4 = sum over h's distinct n-grams g of min(count_h(g), max_j count_j(g))
    4..7   guess_n = max(0, len_h - n + 1)
    8      len_h            9  ref_len: the reference length closest to len_h, the shorter one on a tie
    10     lcs_max = max_j LCS(h, r_j)
    11,12  the (lcs_j, len_j) with the largest lcs_j / len_j (exact integer comparison, lowest j on a tie, references without units
           skipped, (0, 0) when there is none)
    13     the number of present references (0: the row is all zeros)          14, 15  0

The scores are the COCO caption tools' formulas.  With tiny = 1e-15, small = 1e-9, test length c and reference length r:
    ratio   = (c + tiny) / (r + small)
    Bleu_n  = (prod_{k <= n} (match_k + tiny) / (guess_k + small)) ^ (1 / n) * (exp(1 - 1 / ratio) if ratio < 1 else 1)
    ROUGE_L = (1 + beta^2) p q / (q + beta^2 p)  with p = lcs_max / len_h, q = stats[11] / stats[12]; 0 unless both are non-zero
The sentence scores use one row's integers; the corpus BLEU uses the integers summed over the images (c = sum len_h, r = sum
ref_len), the corpus ROUGE_L is the mean of the images' scores.  On sentencepiece ids these are not the published word-level
numbers; on word ids they are (the caveat of scst's CIDEr-D).

Limits: at most 64 units per sequence (L <= 65, Lr <= 64), 1 <= R <= 16 references per image, ids below 65535.  On CUDA tensors
caption_stats is the kernel klab_caption_stats; on CPU tensors the same rule runs on the host in plain Python."""
import math

import torch

from . import ops

MAX_UNITS = 64
MAX_REFS = 16
STATS = 16
TINY, SMALL = 1e-15, 1e-9
SCORES = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L")


def _check(hyp, refs):
    """(B, n) of a valid pair; ValueError otherwise, before anything is enqueued"""
    if not torch.is_tensor(hyp) or hyp.dtype != torch.int64 or hyp.dim() != 2 or hyp.shape[1] < 1:
        raise ValueError(f"hyp has to be an int64 tensor [B * n, L], got {getattr(hyp, 'dtype', type(hyp))} {tuple(getattr(hyp, 'shape', ()))}")
    if hyp.shape[1] > MAX_UNITS + 1:
        raise ValueError(f"hyp holds {hyp.shape[1]} columns; the statistics kernel takes the start token and at most {MAX_UNITS} units")
    if not torch.is_tensor(refs) or refs.dtype != torch.int64 or refs.dim() != 3:
        raise ValueError(f"the references have to be an int64 tensor [B, R, Lr], got {getattr(refs, 'dtype', type(refs))} "
                         f"{tuple(getattr(refs, 'shape', ()))}")
    B, R, Lr = refs.shape
    if not 1 <= R <= MAX_REFS or not 1 <= Lr <= MAX_UNITS:
        raise ValueError(f"references [B, R, Lr] need 1 <= R <= {MAX_REFS} and 1 <= Lr <= {MAX_UNITS}, got {tuple(refs.shape)}")
    if refs.device != hyp.device:
        raise ValueError(f"the references are on {refs.device}, the sequences on {hyp.device}")
    if B < 1 or hyp.shape[0] < 1 or hyp.shape[0] % B:
        raise ValueError(f"hyp holds {hyp.shape[0]} rows, which is no multiple of the {B} images of refs")
    return B, hyp.shape[0] // B


def _check_eos(eos_token_id):
    if not isinstance(eos_token_id, int) or isinstance(eos_token_id, bool) or not 0 <= eos_token_id < 0xFFFF:
        raise ValueError(f"`eos_token_id` has to be an integer in 0..65534, but is {eos_token_id!r}")


# ---- the host path: the kernel's rule in plain Python -------------------------------------------------------------------------------
def _units(row, eos, count_eos):
    out = []
    for t in row:
        if t < 0 or t >= 0xFFFF:
            break
        if t == eos:
            if count_eos:
                out.append(t)
            break
        out.append(t)
    return out


def _lcs(a, b):
    """the kernel's bit-parallel recurrence over b's positions, on a Python integer"""
    if not a or not b:
        return 0
    mask = (1 << len(b)) - 1
    where = {}
    for i, t in enumerate(b):
        where[t] = where.get(t, 0) | 1 << i
    V = mask
    for t in a:
        M = where.get(t, 0)
        U = V & M
        V = ((V + U) | (V & ~M)) & mask
    return bin(~V & mask).count("1")


def _host_row(h, present):
    row = [0] * STATS
    if not present:
        return row
    for n in range(1, 5):
        clip = {}
        for rf in present:
            cnt = {}
            for i in range(len(rf) - n + 1):
                g = tuple(rf[i:i + n])
                cnt[g] = cnt.get(g, 0) + 1
            for g, c in cnt.items():
                if c > clip.get(g, 0):
                    clip[g] = c
        mine = {}
        for i in range(len(h) - n + 1):
            g = tuple(h[i:i + n])
            mine[g] = mine.get(g, 0) + 1
        row[n - 1] = sum(min(c, clip.get(g, 0)) for g, c in mine.items())
        row[3 + n] = max(0, len(h) - n + 1)
    row[8] = len(h)
    row[9] = min((abs(len(rf) - len(h)), len(rf)) for rf in present)[1]
    best = (0, 0)
    for rf in present:
        if not rf:
            continue
        lcs = _lcs(h, rf)
        row[10] = max(row[10], lcs)
        if best[1] == 0 or lcs * best[1] > best[0] * len(rf):
            best = (lcs, len(rf))
    row[11], row[12] = best
    row[13] = len(present)
    return row


def _host_stats(hyp, refs, n, eos, count_eos):
    refs_l = refs.tolist()
    present = [[_units(rf, eos, count_eos) for rf in image if rf[0] >= 0] for image in refs_l]
    rows = [_host_row(_units(h[1:], eos, count_eos), present[r // n]) for r, h in enumerate(hyp.tolist())]
    return torch.tensor(rows, dtype=torch.int32).view(refs.shape[0], n, STATS)


# ---- the public functions ------------------------------------------------------------------------------------------------------------
def caption_stats(hyp, refs, eos_token_id=1, count_eos=False):
    """int32 [B, n, 16]: the statistics (module docstring) of hyp (int64 [B * n, L], or [B, L] with n = 1) against refs (int64
    [B, R, Lr]).  CUDA tensors: one launch of klab_caption_stats, no host read.  CPU tensors: the same integers from the host."""
    B, n = _check(hyp, refs)
    _check_eos(eos_token_id)
    if not hyp.is_cuda:
        return _host_stats(hyp, refs, n, eos_token_id, bool(count_eos))
    stats = torch.empty(B, n, STATS, dtype=torch.int32, device=hyp.device)
    ops.caption_stats(hyp.contiguous(), refs.contiguous(), stats, n_h=n, eos=eos_token_id, count_eos=count_eos)
    return stats


def sentence_scores(stats, beta=1.2):
    """fp64 [..., 5] = Bleu_1, Bleu_2, Bleu_3, Bleu_4, ROUGE_L of every row of stats ([..., 16] integers as caption_stats returns
    them), by element-wise torch operations on stats' own device: no host read.  Rows without a present reference score exactly 0."""
    if not torch.is_tensor(stats) or stats.dim() < 1 or stats.shape[-1] != STATS or stats.dtype.is_floating_point:
        raise ValueError(f"stats has to be an integer tensor [..., {STATS}], got {getattr(stats, 'dtype', type(stats))} "
                         f"{tuple(getattr(stats, 'shape', ()))}")
    if not (isinstance(beta, (int, float)) and math.isfinite(beta) and beta > 0):
        raise ValueError(f"`beta` has to be a finite float > 0, but is {beta}")
    s = stats.to(torch.float64)
    scored = stats[..., 13] > 0
    zero = torch.zeros_like(s[..., 0])
    ratio = (s[..., 8] + TINY) / (s[..., 9] + SMALL)
    penalty = torch.where(ratio < 1, torch.exp(1 - 1 / ratio), torch.ones_like(ratio))
    out = []
    prod = torch.ones_like(ratio)
    for n in range(4):
        prod = prod * ((s[..., n] + TINY) / (s[..., 4 + n] + SMALL))
        out.append(torch.where(scored, torch.pow(prod, 1.0 / (n + 1)) * penalty, zero))
    both = scored & (stats[..., 10] > 0) & (stats[..., 11] > 0)  # p and q non-zero (then len_h and stats[12] are >= 1)
    one = torch.ones_like(zero)
    p = s[..., 10] / torch.where(both, s[..., 8], one)
    q = s[..., 11] / torch.where(both, s[..., 12], one)
    b2 = float(beta) ** 2
    out.append(torch.where(both, (1 + b2) * p * q / torch.where(both, q + b2 * p, one), zero))
    return torch.stack(out, -1)


def corpus_scores(sums):
    """{"Bleu_1" .. "Bleu_4", "ROUGE_L", ["CIDEr-D"], "images"} from CaptionMetrics.sums as a list of 12 (13) host numbers"""
    images = int(sums[11])
    ratio = (sums[8] + TINY) / (sums[9] + SMALL)
    penalty = math.exp(1 - 1 / ratio) if ratio < 1 else 1.0
    out, prod = {}, 1.0
    for n in range(4):
        prod *= (sums[n] + TINY) / (sums[4 + n] + SMALL)
        out[SCORES[n]] = prod ** (1.0 / (n + 1)) * penalty if images else 0.0
    out["ROUGE_L"] = sums[10] / images if images else 0.0
    if len(sums) > 12:
        out["CIDEr-D"] = sums[12] / images if images else 0.0
    out["images"] = images
    return out


class CaptionMetrics:
    """Corpus BLEU-1..4, ROUGE-L (and CIDEr-D with cider=a scst.CiderD) of a validation run, accumulated on the device.

    sums: ONE device tensor, fp64 [12] -- sum match_1..4, sum guess_1..4, sum len_h, sum ref_len, sum ROUGE_L, the number of scored
    images -- and [13] with cider, the last element the sum of the images' CIDEr-D.  It is None until the first update.  It is what
    a data-parallel loop all-reduces (sum) before compute(); integer sums are exact in fp64 up to 2^53.  Images without a present
    reference are skipped.  update() reads nothing from the device; compute() is the one host read."""

    def __init__(self, eos_token_id=1, count_eos=False, cider=None):
        _check_eos(eos_token_id)
        if cider is not None:
            from . import scst
            if not isinstance(cider, scst.CiderD):
                raise ValueError(f"`cider` has to be a scst.CiderD or None, got {type(cider).__name__}")
        self.eos_token_id, self.count_eos, self.cider = eos_token_id, bool(count_eos), cider
        self.sums = None

    def update(self, hyp, refs):
        """adds one batch: hyp int64 [B, L] (one caption per image), refs int64 [B, R, Lr]"""
        if torch.is_tensor(hyp) and hyp.dim() != 2:
            raise ValueError(f"update takes one caption per image, hyp [B, L]; got {tuple(hyp.shape)}")
        B, n = _check(hyp, refs)
        if n != 1:
            raise ValueError(f"update takes one caption per image: hyp holds {hyp.shape[0]} rows for {B} images")
        stats = caption_stats(hyp, refs, self.eos_token_id, self.count_eos).view(B, STATS)
        parts = [stats[:, :10].sum(0, dtype=torch.float64), sentence_scores(stats)[:, 4].sum().view(1),
                 (stats[:, 13] > 0).sum(dtype=torch.float64).view(1)]
        if self.cider is not None:
            from . import scst
            parts.append(scst.ciderd(self.cider, hyp, refs).sum(dtype=torch.float64).view(1))  # (exactly 0 without a present reference)
        batch = torch.cat(parts)
        if self.sums is None:
            self.sums = batch
        else:
            if self.sums.device != batch.device:
                raise ValueError(f"the sums are on {self.sums.device}, this batch on {batch.device}")
            self.sums += batch

    def compute(self):
        """the corpus scores as host floats and the number of scored images (all 0 before the first update)"""
        width = 13 if self.cider is not None else 12
        return corpus_scores([0.0] * width if self.sums is None else self.sums.tolist())

    def reset(self):
        self.sums = None
