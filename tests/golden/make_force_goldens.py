#!/usr/bin/env python3
"""Forced-decoding goldens from the REFERENCE itself (build container only; CPU).

Runs the reference's own ``MyModel`` (ref/models/model.py:8-42) in fp32 on the weights and inputs of ``tiny_b.npz`` (plain and
EOS-biased, the ``tiny_b.eos_row`` of beam.npz, see make_beam_goldens.py) and ``tiny_v11_a.npz`` (rebuilt from the stored weights
as make_logprobs_goldens.py does).  Per model ``<m>`` = ``<name>.<variant>``:

(a) candidate scores: per image N = 5 candidates of L = 6 tokens, as labels are (no start token) -- an EOS at position 1, an EOS
    at position L, a row without EOS, a row with junk after its EOS and a row padded after its EOS.  ``<m>.cand`` int64 [B, N, L];
    ``<m>.cand_logprobs`` f64 [B, N, L] = log_softmax(transformer(inputs_embeds=<the reference's concat>, labels=cand).logits) in
    float64, gathered at the labels (every position; what follows a row's first EOS is not compared by the tests);
    ``<m>.cand_order0`` / ``<m>.cand_order1`` int64 [B, N]: the candidates of each image, best first, by sum / length ** penalty
    for length_penalty 0 and 1 (length = tokens through the first EOS).
(b) decoder prompts: ``transformer.generate(inputs_embeds=..., decoder_input_ids=prompt, max_length=10, use_cache=False)`` -- HF's
    greedy loop -- for a prompt of 1 token and one of 3 tokens that holds an EOS, each plain, with ``min_new_tokens=3`` and with
    ``repetition_penalty=1.3, no_repeat_ngram_size=2``.  ``<case>.prompt`` int64 [B, P] (without the start token, which HF
    prepends), ``<case>.seq`` int64 [B, <= 10].

Guards: every image's candidate scores differ pairwise by more than GAP at both penalties (the ranking is well defined); a float64
rerun of every prompt case gives the same ids; some prompt case goes on generating after the EOS inside its prompt.

Run:  python tests/golden/make_force_goldens.py      -> force.npz + force.json next to this file
"""
import copy
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_beam_goldens import build_dirs, concat_embeds, reference_model  # noqa: E402
from make_logprobs_goldens import build_dirs_v11  # noqa: E402

N, L = 5, 6
MAX_LENGTH = 10
GAP = 1e-3
EOS = 1
MODELS = (("tiny_b", "plain"), ("tiny_b", "eos"), ("tiny_v11_a", "plain"))
PROMPT_KWARGS = (("none", {}), ("minnew", dict(min_new_tokens=3)), ("procs", dict(repetition_penalty=1.3, no_repeat_ngram_size=2)))


def candidates(B, vocab, seed):
    """[B, N, L]: row 0 EOS at position 1 (padded), 1 EOS at position L, 2 no EOS, 3 EOS at position 3 then junk, 4 EOS at position 4
    (padded); every other token is drawn from [2, vocab)"""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(2, vocab, (B, N, L), generator=g)
    c[:, 0, 0] = EOS
    c[:, 0, 1:] = 0
    c[:, 1, L - 1] = EOS
    c[:, 3, 2] = EOS
    c[:, 4, 3] = EOS
    c[:, 4, 4:] = 0
    return c


def lengths(c):
    """tokens through the first EOS (L without one)"""
    hit = c == EOS
    first = torch.where(hit.any(-1), hit.float().argmax(-1) + 1, torch.full(c.shape[:-1], c.shape[-1]))
    return first.long()


def main():
    torch.set_num_threads(4)
    beam = np.load(os.path.join(HERE, "beam.npz"))
    arrays, cases, models = {}, [], []
    past_eos = 0
    for name, variant in MODELS:
        z = np.load(os.path.join(HERE, f"{name}.npz"))
        pix, src = torch.from_numpy(z["pixel_values"]), torch.from_numpy(z["src_ids"])
        root = tempfile.mkdtemp(prefix="klab_force_")
        if name.startswith("tiny_v11"):
            model = reference_model(build_dirs_v11(name, z, root))
            with torch.no_grad():
                ids = model({"pixel_values": pix}, {"input_ids": src}, return_loss=False)
            assert torch.equal(ids, torch.from_numpy(z["greedy_ids"])), "the rebuilt model is not the fixture's"
        else:
            eos_row = torch.from_numpy(beam[f"{name}.eos_row"]) if variant == "eos" else None
            model = reference_model(build_dirs(name, z, root, eos_row))
        shutil.rmtree(root)
        embeds = concat_embeds(model, pix, src)
        B = embeds.shape[0]
        vocab = model.transformer.config.vocab_size
        mid = f"{name}.{variant}"
        # (a) candidate scores
        cand = candidates(B, vocab, 17 + len(models))
        with torch.no_grad():
            logits = model.transformer(inputs_embeds=embeds.repeat_interleave(N, 0), labels=cand.view(B * N, L)).logits
        lp = torch.log_softmax(logits.double(), -1).gather(-1, cand.view(B * N, L, 1)).view(B, N, L)
        ln = lengths(cand)
        live = torch.arange(L).view(1, 1, L) < ln.unsqueeze(-1)
        total = torch.where(live, lp, torch.zeros_like(lp)).sum(-1)
        arrays[mid + ".cand"] = cand.numpy().astype(np.int64)
        arrays[mid + ".cand_logprobs"] = lp.numpy().astype(np.float64)
        for penalty in (0, 1):
            sc = total / ln.double() ** penalty
            gap = (sc.unsqueeze(-1) - sc.unsqueeze(-2)).abs() + torch.eye(N) * 1e9
            assert float(gap.min()) > GAP, (mid, penalty, "two candidates score within GAP", float(gap.min()))
            arrays[mid + f".cand_order{penalty}"] = torch.argsort(sc, -1, descending=True).numpy().astype(np.int64)
        models.append(dict(id=mid, model=name, variant=variant, B=int(B), vocab=int(vocab)))
        print(mid, "candidate scores", total.tolist(), flush=True)
        # (b) decoder prompts
        g = torch.Generator().manual_seed(29 + len(models))
        one = torch.randint(2, vocab, (B, 1), generator=g)
        three = torch.randint(2, vocab, (B, 3), generator=g)
        three[0, 2] = EOS  # a prompt that ends in EOS ...
        three[1:, 1] = EOS  # ... and prompts with an EOS inside
        double = copy.deepcopy(model.transformer).double()
        for pname, prompt in (("p1", one), ("p3", three)):
            for kname, kw in PROMPT_KWARGS:
                with torch.no_grad():
                    seq = model.transformer.generate(inputs_embeds=embeds, decoder_input_ids=prompt, do_sample=False, num_beams=1,
                                                     max_length=MAX_LENGTH, use_cache=False, **kw)
                    again = double.generate(inputs_embeds=embeds.double(), decoder_input_ids=prompt, do_sample=False, num_beams=1,
                                            max_length=MAX_LENGTH, use_cache=False, **kw)
                assert seq.shape == again.shape and torch.equal(seq, again), (mid, pname, kname, "float64 decides differently")
                P = prompt.shape[1]
                assert torch.equal(seq[:, 0], torch.zeros(B, dtype=seq.dtype)) and torch.equal(seq[:, 1:1 + P], prompt)
                if pname == "p3" and seq.shape[1] > 1 + P:
                    past_eos += int(((seq[:, 1 + P:] != 0) & (seq[:, 1 + P:] != EOS)).any())
                cid = f"{mid}.{pname}.{kname}"
                arrays[cid + ".prompt"] = prompt.numpy().astype(np.int64)
                arrays[cid + ".seq"] = seq.numpy().astype(np.int64)
                cases.append(dict(id=cid, model=name, variant=variant, prompt=pname, kwargs=kw, max_length=MAX_LENGTH,
                                  length=int(seq.shape[1])))
                print(cid, seq.tolist(), flush=True)
    assert past_eos > 0, "no row goes on generating after the EOS inside its prompt"
    np.savez_compressed(os.path.join(HERE, "force.npz"), **arrays)
    json.dump(dict(models=models, cases=cases, n=N, length=L, max_length=MAX_LENGTH, gap=GAP), open(os.path.join(HERE, "force.json"), "w"),
              indent=1)
    print("force goldens:", len(models), "models,", len(cases), "prompt cases")


if __name__ == "__main__":
    main()
