#!/usr/bin/env python3
"""Sampling goldens from the REFERENCE itself (build container only; CPU).

Runs the reference's own ``MyModel`` (ref/models/model.py:8-42) on the weights and inputs of ``tiny_a.npz`` / ``tiny_b.npz`` /
``tiny_c.npz``, plain and EOS-biased (the ``<model>.eos_row`` of beam.npz, see make_beam_goldens.py), and calls
``.transformer.generate(inputs_embeds=<the reference's concat>, do_sample=True, output_scores=True,
return_dict_in_generate=True)`` -- HF's ``_sample`` -- over a grid of temperature, top_k, top_p and num_return_sequences, each
case after ``torch.manual_seed(<case index>)``.  Stored per case (rows row0 .. row0 + rows of the stacked arrays): the sampled
sequences (``seq``, padded with -1 to max_length) and, per generated step, the kept set of the processed scores (``kept``,
``np.packbits(scores > -inf)`` along the vocabulary, padded to 512 tokens and max_length - 1 steps).  HF draws with
torch.multinomial, so the sequences are only teacher-forcing inputs for the tests, never an expected output.

Also stored: the warpers' outputs on fixed logits matrices (``warp_x`` [2, 4, 160] and ``warp_out`` [2, grid, 4, 160], the grid
in itertools.product order of TEMPERATURE, TOP_K, TOP_P), which pin the tests' torch restatement (tests/sample_ref.py) to HF's
own classes.

Guards: some case finishes a row with EOS; some case's rows of one image differ; every top_p < 1 case removes a token somewhere.

Run:  python tests/golden/make_sample_goldens.py      -> sample.npz + sample.json next to this file
"""
import itertools
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

MODELS = ("tiny_a", "tiny_b", "tiny_c")
TEMPERATURE = (0.7, 1.0, 1.5)
TOP_K = (0, 1, 5, 50)
TOP_P = (1.0, 0.9, 0.5)
NUM_RETURN = (1, 3)
MAX_LENGTH = 8


def warper_goldens(arrays):
    from transformers.generation.logits_process import LogitsProcessorList, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    g = torch.Generator().manual_seed(11)
    mats = [torch.randn(4, 160, generator=g) * 3.0, (torch.randn(4, 160, generator=g) * 2.0).round()]  # the second one full of ties
    outs = []
    for x in mats:
        outs.append([])
        for t, k, p in itertools.product(TEMPERATURE, TOP_K, TOP_P):
            procs = LogitsProcessorList()  # the construction and order of generation/utils.py for do_sample=True, num_beams=1
            if t != 1.0:
                procs.append(TemperatureLogitsWarper(t))
            if k != 0:
                procs.append(TopKLogitsWarper(top_k=k, min_tokens_to_keep=1))
            if p < 1.0:
                procs.append(TopPLogitsWarper(top_p=p, min_tokens_to_keep=1))
            outs[-1].append(procs(None, x.clone()).numpy())
    arrays["warp_x"] = torch.stack(mats).numpy()
    arrays["warp_out"] = np.stack([np.stack(o) for o in outs])


def main():
    torch.set_num_threads(4)
    beam = np.load(os.path.join(HERE, "beam.npz"))
    arrays, cases, seqs, kepts = {}, [], [], []
    warper_goldens(arrays)
    saw_eos = saw_diverse = False
    idx = 0
    for name in MODELS:
        z = np.load(os.path.join(HERE, f"{name}.npz"))
        pix, src = torch.from_numpy(z["pixel_values"]), torch.from_numpy(z["src_ids"])
        for variant in ("plain", "eos"):
            root = tempfile.mkdtemp(prefix="klab_sample_")
            eos_row = torch.from_numpy(beam[f"{name}.eos_row"]) if variant == "eos" else None
            model = reference_model(build_dirs(name, z, root, eos_row))
            shutil.rmtree(root)
            embeds = concat_embeds(model, pix, src)
            for t, k, p, n in itertools.product(TEMPERATURE, TOP_K, TOP_P, NUM_RETURN):
                torch.manual_seed(idx)
                idx += 1
                with torch.no_grad():
                    out = model.transformer.generate(inputs_embeds=embeds, do_sample=True, temperature=t, top_k=k, top_p=p,
                                                     num_return_sequences=n, max_length=MAX_LENGTH, use_cache=False,
                                                     output_scores=True, return_dict_in_generate=True)
                seq = out.sequences
                kept = torch.stack([s > -float("inf") for s in out.scores], 1).numpy()  # [rows, steps, V]
                if p < 1.0:
                    assert not kept.all(), (name, variant, t, k, p, n)
                saw_eos |= bool((seq[:, 1:] == 1).any())
                if n > 1:
                    saw_diverse |= any(len({tuple(r) for r in seq[b * n:(b + 1) * n].tolist()}) > 1 for b in range(src.shape[0]))
                cid = f"{name}.{variant}.t{t}.k{k}.p{p}.n{n}"
                rows, steps = seq.shape[0], seq.shape[1] - 1
                sp = np.full((rows, MAX_LENGTH), -1, dtype=np.int64)
                sp[:, :seq.shape[1]] = seq.numpy()
                kp = np.zeros((rows, MAX_LENGTH - 1, 64), dtype=np.uint8)
                kp[:, :steps, :kept.shape[-1] // 8] = np.packbits(kept, axis=-1)
                cases.append(dict(id=cid, model=name, variant=variant, temperature=t, top_k=k, top_p=p, num_return_sequences=n,
                                  max_length=MAX_LENGTH, vocab=int(kept.shape[-1]), row0=sum(len(a) for a in seqs), rows=rows,
                                  length=int(seq.shape[1])))
                seqs.append(sp)
                kepts.append(kp)
            print(name, variant, "cases so far", len(cases), flush=True)
    assert saw_eos, "no sampled row ever finishes with EOS"
    assert saw_diverse, "the rows of one image never differ"
    arrays["seq"] = np.concatenate(seqs)
    arrays["kept"] = np.concatenate(kepts)
    np.savez_compressed(os.path.join(HERE, "sample.npz"), **arrays)
    json.dump(dict(cases=cases, max_length=MAX_LENGTH, warp=dict(temperature=TEMPERATURE, top_k=TOP_K, top_p=TOP_P, matrices=2)),
              open(os.path.join(HERE, "sample.json"), "w"), indent=1)
    print("sample goldens:", len(cases), "cases")


if __name__ == "__main__":
    main()
