"""Self-critical sequence training (Rennie et al.) for the native captioner: sample captions, reward them with CIDEr-D against the
image's reference captions, train on -(reward - baseline) log p(sample) -- rewards, labels, weights and advantages all on the device.

    table = scst.CiderD.from_references(refs, vocab_size=V, eos_token_id=1)   # once per dataset; refs: per image a list of id lists
    table.to("cuda")
    sc = scst.SelfCritical(model, table, samples=5, baseline="greedy", max_length=20)
    loss, info = sc.loss(images, source_encoding, refs_tensor)                 # refs_tensor int64 [B, R, Lr], label format
    loss.backward(); opt.step()

SelfCritical(..., reward_weights={"ciderd": 1.0, "bleu4": 0.5}) mixes the reward with the sentence BLEU-4 and ROUGE-L of metrics.py.

CIDEr-D (Vedantam et al.; the CiderD scorer of the COCO caption tools) is computed over units = token ids, so it equals the COCO
tools' number only on word-id sequences.  A sequence's units are its tokens through the first EOS -- the EOS itself is a unit when
count_eos (the default: it rewards ending the caption) -- and an id < 0 or >= 0xFFFF ends it.  Id lists given to from_references
follow the same rule: pass them as the label rows hold them, closed by EOS.  Document frequency counts IMAGES, not references.

Limits: at most 64 units per sequence (max_length <= 65, Lr <= 64), 1 <= R <= 16 references per image, vocab_size <= 65535.
Sampling and training use different bindings of the engine, so a step re-binds twice and runs the Swin tower and the encoders once
per decoding session as well as once in the training forward (DESIGN.md section 24 has the measured cost).  No beam-search samples."""
import itertools
import math

import numpy as np
import torch

from . import metrics, ops

MAX_UNITS = 64
MAX_REFS = 16
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
BASELINES = {"greedy": 0, "mean": 1, "none": 2}  # klab_scst_targets' modes
REWARD_TERMS = ("ciderd", "bleu4", "rouge_l")     # SelfCritical's reward_weights, in the order the mixture adds them


def _home_slots(keys, cap):
    """(key * GOLDEN mod 2^64) >> (64 - log2 cap) of a uint64 array"""
    with np.errstate(over="ignore"):
        return ((keys * GOLDEN) >> np.uint64(64 - (cap.bit_length() - 1))).astype(np.int64)


class CiderD:
    """The document-frequency table of a reference corpus as the device kernel reads it: keys uint64 [cap] (stored as int64 bits;
    all ones = empty slot) and idf fp32 [cap], cap a power of two >= 2x the entries, open addressing with linear probing."""

    def __init__(self, keys, idf, n_images, entries, vocab_size, eos_token_id, count_eos, sigma):
        self.keys, self.idf = keys, idf
        self.n_images, self.entries = int(n_images), int(entries)
        self.vocab_size, self.eos_token_id = int(vocab_size), int(eos_token_id)
        self.count_eos, self.sigma = bool(count_eos), float(sigma)
        self.log_n = float(np.float32(math.log(self.n_images)))  # the weight of an n-gram no reference holds

    @property
    def capacity(self):
        return self.keys.numel()

    @property
    def device(self):
        return self.keys.device

    @classmethod
    def from_references(cls, refs, vocab_size, eos_token_id=1, count_eos=True, sigma=6.0, capacity=None):
        """refs: per image a list of id lists (its reference captions).  Runs on the host in numpy; idf = log N - log max(1, df) in
        fp64, rounded to fp32 once.  capacity (tests): the number of slots, a power of two >= 2x the entries."""
        V, eos = int(vocab_size), int(eos_token_id)
        if not 0 < V <= 0xFFFF:
            raise ValueError(f"`vocab_size` has to be in 1..65535 (an n-gram's key packs four 16-bit ids), but is {vocab_size}")
        if not 0 <= eos < V:
            raise ValueError(f"`eos_token_id` ({eos_token_id}) is outside the vocabulary of {V}")
        if not (isinstance(sigma, (int, float)) and math.isfinite(sigma) and sigma > 0):
            raise ValueError(f"`sigma` has to be a finite float > 0, but is {sigma}")
        n_images = len(refs)
        if n_images < 1:
            raise ValueError("from_references needs the references of at least one image")
        caps = [c for im in refs for c in im]
        lens = np.fromiter((len(c) for c in caps), np.int64, len(caps))
        image = np.repeat(np.arange(n_images), np.fromiter((len(im) for im in refs), np.int64, n_images))
        width = int(lens.max()) if len(caps) else 0
        tok = np.full((len(caps), width + 3), -1, np.int64)
        flat = np.fromiter(itertools.chain.from_iterable(caps), np.int64, int(lens.sum()))
        if flat.size and (flat.min() < 0 or flat.max() >= V):
            raise ValueError(f"refs holds ids outside [0, {V})")
        start = np.cumsum(lens) - lens
        tok[np.repeat(np.arange(len(caps)), lens), np.arange(flat.size) - np.repeat(start, lens)] = flat
        # units: through the first EOS (a pad of -1 ends a caption without one)
        stop = (tok < 0) | (tok == eos)
        first = stop.argmax(1)
        units = first + ((tok[np.arange(len(caps)), first] == eos) & bool(count_eos)) if len(caps) else lens
        if len(caps) and int(units.max()) > MAX_UNITS:
            raise ValueError(f"a reference holds {int(units.max())} units; the reward kernel takes at most {MAX_UNITS}")
        col = np.arange(width)
        t16 = np.where(tok < 0, 0xFFFF, tok).astype(np.uint64)
        all_keys, all_img = [], []
        for n in range(1, 5):
            key = np.zeros((len(caps), width), np.uint64)
            for k in range(4):
                key |= (t16[:, k:k + width] if k < n else np.uint64(0xFFFF)) << np.uint64(16 * k)
            inside = col[None, :] + n <= units[:, None]
            all_keys.append(key[inside])
            all_img.append(np.broadcast_to(image[:, None], key.shape)[inside])
        key, img = np.concatenate(all_keys), np.concatenate(all_img)
        order = np.lexsort((img, key))
        key, img = key[order], img[order]
        once = np.ones(key.size, bool)  # one (n-gram, image) pair each: several references of an image count once
        once[1:] = (key[1:] != key[:-1]) | (img[1:] != img[:-1])
        ukeys, df = np.unique(key[once], return_counts=True)
        idf = (math.log(n_images) - np.log(np.maximum(1, df).astype(np.float64))).astype(np.float32)
        need = max(2, 1 << max(0, (2 * ukeys.size - 1)).bit_length())
        if capacity is None:
            capacity = need
        capacity = int(capacity)
        if capacity < 2 or capacity & (capacity - 1) or capacity < 2 * ukeys.size:
            raise ValueError(f"`capacity` ({capacity}) has to be a power of two >= 2x the {ukeys.size} entries")
        tkeys = np.full(capacity, EMPTY, np.uint64)
        tidf = np.zeros(capacity, np.float32)
        # vectorised probing rounds: of the pending keys that look at a free slot the first per slot takes it; whoever looks at a
        # taken slot moves one on (with wrap-around), so every slot between a key's home and its place is taken
        slot = _home_slots(ukeys, capacity)
        pending = np.arange(ukeys.size)
        while pending.size:
            s = slot[pending]
            free = tkeys[s] == EMPTY
            _u, firsts = np.unique(s[free], return_index=True)
            win = pending[free][firsts]
            tkeys[slot[win]] = ukeys[win]
            tidf[slot[win]] = idf[win]
            placed = np.zeros(ukeys.size, bool)
            placed[win] = True
            pending = pending[~placed[pending]]
            slot[pending] = (slot[pending] + 1) & (capacity - 1)
        return cls(torch.from_numpy(tkeys.view(np.int64)), torch.from_numpy(tidf), n_images, ukeys.size, V, eos, count_eos, sigma)

    def to(self, device):
        """moves the two arrays (in place) and returns the table"""
        self.keys, self.idf = self.keys.to(device), self.idf.to(device)
        return self

    def state_dict(self):
        return dict(keys=self.keys.cpu(), idf=self.idf.cpu(), n_images=self.n_images, entries=self.entries, vocab_size=self.vocab_size,
                    eos_token_id=self.eos_token_id, count_eos=self.count_eos, sigma=self.sigma)

    @classmethod
    def from_state_dict(cls, sd):
        keys, idf = torch.as_tensor(sd["keys"]), torch.as_tensor(sd["idf"])
        cap = keys.numel()
        if keys.dtype != torch.int64 or idf.dtype != torch.float32 or idf.numel() != cap or cap < 2 or cap & (cap - 1):
            raise ValueError("CiderD state: keys int64 [cap] and idf float32 [cap] with cap a power of two are needed")
        return cls(keys.clone(), idf.clone(), sd["n_images"], sd["entries"], sd["vocab_size"], sd["eos_token_id"], sd["count_eos"], sd["sigma"])


def _check_refs(table, refs, B, device):
    if not isinstance(table, CiderD):
        raise ValueError(f"`table` has to be a scst.CiderD, got {type(table).__name__}")
    if not torch.is_tensor(refs) or refs.dtype != torch.int64 or refs.dim() != 3 or refs.shape[0] != B:
        raise ValueError(f"the references have to be an int64 tensor [B, R, Lr] with B = {B}, got "
                         f"{getattr(refs, 'dtype', type(refs))} {tuple(getattr(refs, 'shape', ()))}")
    if not 1 <= refs.shape[1] <= MAX_REFS or not 1 <= refs.shape[2] <= MAX_UNITS:
        raise ValueError(f"references [B, R, Lr] need 1 <= R <= {MAX_REFS} and 1 <= Lr <= {MAX_UNITS}, got {tuple(refs.shape)}")
    if refs.device != device or table.device != device:
        raise ValueError(f"the references are on {refs.device} and the table on {table.device}, the sequences on {device}")


def ciderd(table, hyp, refs):
    """CIDEr-D rewards fp32 [B, n] of hyp (int64 [B * n, L] as generate returns them: start token first, image-major) against refs
    (int64 [B, R, Lr] in label format: rows closed by EOS, an absent reference starts with -100).  One launch, no host read; also a
    validation metric (the corpus score is the mean over the images' hypotheses)."""
    if not torch.is_tensor(hyp) or hyp.dtype != torch.int64 or hyp.dim() != 2 or hyp.shape[1] < 1:
        raise ValueError(f"hyp has to be an int64 tensor [B * n, L], got {getattr(hyp, 'dtype', type(hyp))} {tuple(getattr(hyp, 'shape', ()))}")
    if hyp.shape[1] > MAX_UNITS + 1:
        raise ValueError(f"hyp holds {hyp.shape[1]} columns; the reward kernel takes the start token and at most {MAX_UNITS} units")
    B = refs.shape[0] if torch.is_tensor(refs) and refs.dim() == 3 else 0
    _check_refs(table, refs, B, hyp.device)
    if B < 1 or hyp.shape[0] % B:
        raise ValueError(f"hyp holds {hyp.shape[0]} rows, which is no multiple of the {B} images of refs")
    n = hyp.shape[0] // B
    out = torch.empty(B * n, dtype=torch.float32, device=hyp.device)
    ops.ciderd_rewards(hyp.contiguous(), refs.contiguous(), table.keys, table.idf, table.log_n, out, n_h=n, sigma=table.sigma,
                       eos=table.eos_token_id, count_eos=table.count_eos)
    return out.view(B, n)


class SelfCritical:
    """One self-critical step's loss for a MyModel.  baseline: "greedy" (the reward of the greedy caption, Rennie et al.), "mean" (the
    mean reward of the image's other samples, leave-one-out) or "none".

    reward_weights: None (the reward is CIDEr-D, exactly the launches above) or a dict over "ciderd", "bleu4", "rouge_l" with
    finite weights, at least one non-zero: the reward is (w_c * ciderd.double() + w_b * Bleu_4 + w_r * ROUGE_L).float(), the
    sentence scores of metrics.sentence_scores under the table's eos_token_id and count_eos, added in that order; a term with
    weight 0 (or left out) is not computed.  The greedy baseline is scored with the same mixture."""

    def __init__(self, model, table, samples=5, baseline="greedy", max_length=20, temperature=1.0, top_k=0, top_p=1.0,
                 reward_weights=None):
        if not isinstance(table, CiderD):
            raise ValueError(f"`table` has to be a scst.CiderD, got {type(table).__name__}")
        if baseline not in BASELINES:
            raise ValueError(f"`baseline` has to be one of {sorted(BASELINES)}, but is {baseline!r}")
        if not isinstance(samples, int) or samples < 1:
            raise ValueError(f"`samples` has to be a positive integer, but is {samples}")
        if baseline == "mean" and samples < 2:
            raise ValueError("baseline='mean' is the mean of the image's OTHER samples: it needs samples >= 2")
        if not isinstance(max_length, int) or not 2 <= max_length <= MAX_UNITS + 1:
            raise ValueError(f"`max_length` has to be an integer in 2..{MAX_UNITS + 1} (the start token and at most {MAX_UNITS} units), "
                             f"but is {max_length}")
        cfg = model.main_cfg
        if table.vocab_size != cfg.vocab_size or table.eos_token_id != cfg.eos_token_id:
            raise ValueError(f"the table was built for vocab_size {table.vocab_size} / eos {table.eos_token_id}, the model has "
                             f"{cfg.vocab_size} / {cfg.eos_token_id}")
        self.model, self.table = model, table
        self.samples, self.baseline, self.max_length = samples, baseline, max_length
        self.temperature, self.top_k, self.top_p = temperature, top_k, top_p
        if reward_weights is not None:
            if not isinstance(reward_weights, dict) or set(reward_weights) - set(REWARD_TERMS):
                raise ValueError(f"`reward_weights` has to be None or a dict over {REWARD_TERMS}, but is {reward_weights!r}")
            if not all(isinstance(w, (int, float)) and not isinstance(w, bool) and math.isfinite(w) for w in reward_weights.values()):
                raise ValueError(f"`reward_weights` needs finite numbers, but is {reward_weights!r}")
            if not any(w != 0 for w in reward_weights.values()):
                raise ValueError("`reward_weights` needs at least one non-zero weight")
            reward_weights = {k: float(reward_weights.get(k, 0.0)) for k in REWARD_TERMS}
        self.reward_weights = reward_weights

    def _mixture(self, seq, refs, n):
        """(reward fp32 [B * n], {term: its unmixed [B, n] values}) of seq under reward_weights; no host read"""
        table, w = self.table, self.reward_weights
        B = refs.shape[0]
        terms, mix = {}, None
        if w["ciderd"] != 0:
            c = torch.empty(B * n, dtype=torch.float32, device=seq.device)
            ops.ciderd_rewards(seq, refs, table.keys, table.idf, table.log_n, c, n_h=n, sigma=table.sigma, eos=table.eos_token_id,
                               count_eos=table.count_eos)
            terms["ciderd"] = c.view(B, n)
        if w["bleu4"] != 0 or w["rouge_l"] != 0:
            scores = metrics.sentence_scores(metrics.caption_stats(seq, refs, table.eos_token_id, table.count_eos))
            if w["bleu4"] != 0:
                terms["bleu4"] = scores[..., 3]
            if w["rouge_l"] != 0:
                terms["rouge_l"] = scores[..., 4]
        for k in REWARD_TERMS:
            if k in terms:
                part = w[k] * terms[k].double()
                mix = part if mix is None else mix + part
        return mix.float().reshape(-1).contiguous(), terms

    def loss(self, images, source_encoding, refs):
        """(loss, info): loss = sum_t A log-likelihood terms / N over the sampled captions' N scored tokens, i.e. the model's weighted
        forward on the samples as labels with the advantages as weights and weight_norm="count"; info = dict(rewards [B, n],
        baseline [B] (greedy) or None, advantages [B, n], sequences [B * n, L]; with reward_weights also reward_terms, the unmixed
        [B, n] terms of the samples' reward).  Nothing is read from the device beyond generate's stop word per step."""
        model, table, n = self.model, self.table, self.samples
        pixels, src = images["pixel_values"], source_encoding["input_ids"]
        B = src.shape[0]
        _check_refs(table, refs, B, src.device)
        refs = refs.contiguous()
        eos = table.eos_token_id
        model._join_pending_update()  # as MyModel.forward does ahead of its own generate: the sessions read the weights
        model._join_pending_reduce()
        pixels, src = pixels.to(torch.float32).contiguous(), src.to(torch.int64).contiguous()
        was_training = model.transformer.training
        model.transformer.eval()
        try:
            seq = model.generate(pixels, src, max_length=self.max_length, do_sample=True, num_return_sequences=n,
                                 temperature=self.temperature, top_k=self.top_k, top_p=self.top_p)
            greedy = model.generate(pixels, src, max_length=self.max_length) if self.baseline == "greedy" else None
        finally:
            model.transformer.train(was_training)
        dev = seq.device
        base, terms = None, None
        if self.reward_weights is None:
            rewards = torch.empty(B * n, dtype=torch.float32, device=dev)
            ops.ciderd_rewards(seq, refs, table.keys, table.idf, table.log_n, rewards, n_h=n, sigma=table.sigma, eos=eos,
                               count_eos=table.count_eos)
            if greedy is not None:
                base = torch.empty(B, dtype=torch.float32, device=dev)
                ops.ciderd_rewards(greedy, refs, table.keys, table.idf, table.log_n, base, n_h=1, sigma=table.sigma, eos=eos,
                                   count_eos=table.count_eos)
        else:
            rewards, terms = self._mixture(seq, refs, n)
            if greedy is not None:
                base = self._mixture(greedy, refs, 1)[0]
        Lt = self.max_length - 1
        labels = torch.empty(B, n, Lt, dtype=torch.int64, device=dev)
        weights = torch.empty(B, n, Lt, dtype=torch.float32, device=dev)
        adv = torch.empty(B, n, dtype=torch.float32, device=dev)
        ops.scst_targets(seq, rewards, base, labels, weights, adv, n=n, mode=BASELINES[self.baseline], eos=eos)
        saved = model._weight_norm
        model._weight_norm = "count"  # for this call only: the user's setting comes back, on exceptions too
        try:
            loss = model(images, source_encoding, {"input_ids": labels, "loss_weights": weights})
        finally:
            model._weight_norm = saved
        info = dict(rewards=rewards.view(B, n), baseline=base, advantages=adv, sequences=seq)
        if terms is not None:
            info["reward_terms"] = terms
        return loss, info
