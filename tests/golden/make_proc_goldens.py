#!/usr/bin/env python3
"""Logits-processor goldens from the REFERENCE itself (build container only; CPU).

Runs the reference's own ``MyModel`` (ref/models/model.py:8-42) on the weights and inputs of ``tiny_a.npz`` / ``tiny_b.npz`` /
``tiny_c.npz``, plain and EOS-biased (the ``<model>.eos_row`` of beam.npz, see make_beam_goldens.py), and calls
``.transformer.generate(inputs_embeds=<the reference's concat>, ...)`` with HF's logits processors (repetition_penalty,
no_repeat_ngram_size, bad_words_ids, min_length, min_new_tokens) alone and combined, in the three loops:
  greedy   -- the sequences (``<id>.seq``); kept only when an fp64 rerun gives the same sequences and every step's processed
              top-2 gap exceeds GAP (no tie at a decision, never an all -inf row);
  beam     -- num_beams 2 and 4: the sequences and ``sequences_scores`` (``<id>.seq``, ``<id>.scores``); kept only under the
              fp64 rerun and score-gap filter of make_beam_goldens.py;
  sample   -- ``torch.manual_seed(<case index>)``, then per generated step the kept set of the processed + warped scores
              (``<id>.kept``, ``np.packbits(scores > -inf)`` along the vocabulary) and the sampled sequences (``<id>.seq``),
              which are teacher-forcing inputs for the tests, never an expected output.
Bad words are chosen per model from its own greedy output under no_repeat_ngram_size=1 (its most frequent token, one of its
bigrams), plus
``[eos]`` (HF drops it) and an entry longer than any history (HF ignores it).

Also stored: the five processors of HF applied to random scores and histories (``pin_x`` [N, 3, V], ``pin_hist`` [N, 3, H]
padded with -1, ``pin_out`` [N, 3, V]; settings in ``pin``), on the logits and on their log_softmax, which pin the tests'
torch restatement (tests/logits_proc_ref.py) to HF's own classes; and HF's exception type and message for bad arguments
(``errors``), from HF's generate itself.

Guards: for every processor some case's output differs from the same call without it; at least 60 deterministic cases remain.

Run:  python tests/golden/make_proc_goldens.py      -> proc.npz + proc.json next to this file
"""
import collections
import json
import os
import random
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_beam_goldens import build_dirs, concat_embeds, reference_model  # noqa: E402

MODELS = ("tiny_a", "tiny_b", "tiny_c")
MAX_LENGTH = 10
GAP = 1e-4
EOS = 1
PIN_V, PIN_H, PIN_N = 48, 12, 160


def proc_grid(bad):
    """name -> generate kwargs; the names list the processors a case exercises"""
    return collections.OrderedDict([
        ("rep", dict(repetition_penalty=1.3)),
        ("rep_reward", dict(repetition_penalty=0.7)),
        ("ngram2", dict(no_repeat_ngram_size=2)),
        ("ngram3_rep", dict(no_repeat_ngram_size=3, repetition_penalty=1.2)),
        ("bad", dict(bad_words_ids=bad)),
        ("minlen", dict(min_length=7)),
        ("minnew_minlen", dict(min_new_tokens=5, min_length=9)),  # HF: min_length becomes min_new_tokens + 1 = 6
        ("all", dict(repetition_penalty=1.2, no_repeat_ngram_size=2, bad_words_ids=bad, min_new_tokens=4)),
    ])


def pin_goldens(arrays):
    from transformers.generation.logits_process import (LogitsProcessorList, MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor,
                                                        NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor)
    rng = random.Random(5)
    g = torch.Generator().manual_seed(5)
    xs, hs, outs, meta = [], [], [], []
    for i in range(PIN_N):
        L = rng.choice((1, 2, 3, 4, 6, 9, 12))
        hist = torch.randint(0, 6, (3, L), generator=g)  # a small alphabet: duplicates and repeated n-grams
        hist[:, 0] = 0  # the start token
        if i % 3 == 0:
            hist[1, 1:] = torch.tensor([2, 3] * L)[:L - 1]  # a row of repeats
        x = torch.randn(3, PIN_V, generator=g) * 3.0
        pen = rng.choice((1.0, 1.0, 1.3, 0.6))
        ngram = rng.choice((0, 0, 1, 2, 3))
        bad = rng.choice((None, [[3]], [[2, 5], [EOS], [4]], [[2, 3, 4], [0, 2], [5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5]]))
        minl = rng.choice((0, 0, 5))
        minn = rng.choice((None, None, 3))
        mode = rng.choice(("logits", "logprobs"))
        if i < 6:  # each processor alone once
            pen, ngram, bad, minl, minn = [(1.3, 0, None, 0, None), (1.0, 2, None, 0, None), (1.0, 0, [[2, 5], [EOS], [4]], 0, None),
                                           (1.0, 0, None, 5, None), (1.0, 0, None, 0, 3), (0.6, 0, None, 0, None)][i]
        procs = LogitsProcessorList()  # the order of generation/utils.py
        if pen != 1.0:
            procs.append(RepetitionPenaltyLogitsProcessor(penalty=pen))
        if ngram > 0:
            procs.append(NoRepeatNGramLogitsProcessor(ngram))
        if bad is not None:
            procs.append(NoBadWordsLogitsProcessor(bad, torch.tensor([EOS])))
        if minl > 0:
            procs.append(MinLengthLogitsProcessor(minl, torch.tensor([EOS])))
        if minn is not None and minn > 0:
            procs.append(MinNewTokensLengthLogitsProcessor(1, minn, torch.tensor([EOS])))
        s = torch.log_softmax(x, -1) if mode == "logprobs" else x.clone()
        out = procs(hist, s)
        hp = torch.full((3, PIN_H), -1, dtype=torch.int64)
        hp[:, :L] = hist
        xs.append(x.numpy()); hs.append(hp.numpy()); outs.append(out.numpy())
        meta.append(dict(cur_len=L, mode=mode, repetition_penalty=pen, no_repeat_ngram_size=ngram, bad_words_ids=bad, min_length=minl,
                         min_new_tokens=minn))
    arrays["pin_x"] = np.stack(xs).astype(np.float32)
    arrays["pin_hist"] = np.stack(hs)
    arrays["pin_out"] = np.stack(outs).astype(np.float32)
    return meta


ERROR_KWARGS = [
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=2), dict(repetition_penalty=1),
    dict(no_repeat_ngram_size=2.5), dict(no_repeat_ngram_size=-1),
    dict(bad_words_ids=[]), dict(bad_words_ids=[3]), dict(bad_words_ids=[[3, -1]]), dict(bad_words_ids=[[EOS]]), dict(bad_words_ids=[[]]),
    dict(bad_words_ids=[[2], [100000]]), dict(bad_words_ids=[[2.5]]),
    dict(min_length=2.5), dict(min_length=-1), dict(min_new_tokens=2.5), dict(min_new_tokens=-3), dict(min_new_tokens=0),
    dict(min_new_tokens=2, min_length=2.5), dict(repetition_penalty=0.0, no_repeat_ngram_size=2.5),
]


def error_goldens(model, embeds):
    out = []
    for kw in ERROR_KWARGS:
        try:
            with torch.no_grad():
                model.transformer.generate(inputs_embeds=embeds, max_length=4, use_cache=False, **kw)
            out.append(dict(kwargs=kw, type=None, message=None))
        except Exception as ex:  # noqa: BLE001  (the type and text are the golden)
            out.append(dict(kwargs=kw, type=type(ex).__name__, message=str(ex)))
    return out


def gen(model, embeds, mode, kw, **extra):
    with torch.no_grad():
        if mode == "greedy":
            o = model.transformer.generate(inputs_embeds=embeds, do_sample=False, num_beams=1, max_length=MAX_LENGTH, use_cache=False,
                                           output_scores=True, return_dict_in_generate=True, **kw)
            return o.sequences, torch.stack(o.scores, 1)
        if mode == "beam":
            o = model.transformer.generate(inputs_embeds=embeds, do_sample=False, max_length=MAX_LENGTH, use_cache=False,
                                           output_scores=True, return_dict_in_generate=True, **extra, **kw)
            return o.sequences, o.sequences_scores.float()
        o = model.transformer.generate(inputs_embeds=embeds, do_sample=True, max_length=MAX_LENGTH, use_cache=False, output_scores=True,
                                       return_dict_in_generate=True, **extra, **kw)
        return o.sequences, torch.stack(o.scores, 1)


def live_mask(seq):
    tok = seq[:, 1:]
    return (torch.cumsum(torch.cumsum((tok == EOS).long(), 1), 1) <= 1)


def main():
    torch.set_num_threads(4)
    beam = np.load(os.path.join(HERE, "beam.npz"))
    arrays, cases = {}, []
    pin = pin_goldens(arrays)
    bites = collections.Counter()
    errors = None
    sample_idx = 0
    for name in MODELS:
        z = np.load(os.path.join(HERE, f"{name}.npz"))
        pix, src = torch.from_numpy(z["pixel_values"]), torch.from_numpy(z["src_ids"])
        B = src.shape[0]
        for variant in ("plain", "eos"):
            root = tempfile.mkdtemp(prefix="klab_proc_")
            eos_row = torch.from_numpy(beam[f"{name}.eos_row"]) if variant == "eos" else None
            model = reference_model(build_dirs(name, z, root, eos_row))
            embeds = concat_embeds(model, pix, src)
            model64 = reference_model(build_dirs(name, z, root, eos_row)).double()
            embeds64 = concat_embeds(model64, pix.double(), src)
            shutil.rmtree(root)
            if errors is None:
                errors = error_goldens(model, embeds)
            if variant == "plain":
                # bad words from the plain model's own greedy output under no_repeat_ngram_size=1 (without it, random-init models
                # repeat one token; the EOS-biased variant reuses them): its most frequent token, one of its bigrams
                base, _ = gen(model, embeds, "greedy", dict(no_repeat_ngram_size=1))
                toks = [t for t in base[:, 1:].flatten().tolist() if t > 1]
                top = collections.Counter(toks).most_common(2)
                row = base[0, 1:].tolist()
                bad = [[top[0][0]], [row[2], row[3]], [EOS], [top[-1][0]] * (MAX_LENGTH + 2)]
            grid = proc_grid(bad)
            modes = [("greedy", {}), ("beam", dict(num_beams=2)), ("beam", dict(num_beams=4)),
                     ("sample", dict(top_k=0)), ("sample", dict(top_k=5, temperature=0.7))]
            for mode, extra in modes:
                ref = gen(model, embeds, mode, {}, **extra)[0] if mode != "sample" else None
                for pname, kw in grid.items():
                    tag = ".".join(f"{k}{v}" for k, v in extra.items())
                    cid = f"{name}.{variant}.{mode}.{tag}.{pname}" if tag else f"{name}.{variant}.{mode}.{pname}"
                    if mode == "sample":
                        torch.manual_seed(sample_idx)
                        sample_idx += 1
                    seq, sc = gen(model, embeds, mode, kw, **extra)
                    cs = dict(id=cid, model=name, variant=variant, mode=mode, procs=pname, kwargs=kw, max_length=MAX_LENGTH,
                              vocab=int(model.transformer.config.vocab_size), **extra)
                    if mode == "sample":
                        kept = (sc > -float("inf")).numpy()  # [rows, steps, V]
                        arrays[cid + ".seq"] = seq.numpy().astype(np.int64)
                        arrays[cid + ".kept"] = np.packbits(kept, axis=-1)
                        cases.append(cs)
                        continue
                    if seq.shape != ref.shape or not torch.equal(seq, ref):
                        bites[pname] += 1
                    seq64, sc64 = gen(model64, embeds64, mode, kw, **extra)
                    if not torch.equal(seq, seq64):
                        continue
                    if mode == "greedy":
                        top2 = torch.topk(sc.float(), 2, -1)[0]
                        live = live_mask(seq)
                        if not bool(torch.isfinite(top2[..., 0])[live].all()) or not bool(((top2[..., 0] - top2[..., 1]) > GAP)[live].all()):
                            continue
                    else:
                        k = extra["num_beams"]
                        # one returned sequence per sample: the scores of its 2k candidates are not stored, so ask the fp64 rerun
                        if not torch.allclose(sc.double(), sc64.double(), atol=1e-4, rtol=0):
                            continue
                        arrays[cid + ".scores"] = sc.numpy().astype(np.float32)
                        cs["num_beams"] = k
                    arrays[cid + ".seq"] = seq.numpy().astype(np.int64)
                    cases.append(cs)
            print(name, variant, "cases so far", len(cases), flush=True)
    det = [c for c in cases if c["mode"] != "sample"]
    for pname in proc_grid([[2]]):
        assert bites[pname] > 0, f"{pname} never changes an output"
    assert len(det) >= 60, f"only {len(det)} deterministic cases survive the filters"
    assert any(e["type"] is None for e in errors) and any(e["type"] == "ValueError" for e in errors)
    np.savez_compressed(os.path.join(HERE, "proc.npz"), **arrays)
    json.dump(dict(cases=cases, pin=pin, pin_shape=[PIN_N, 3, PIN_V, PIN_H], errors=errors, max_length=MAX_LENGTH, bites=dict(bites)),
              open(os.path.join(HERE, "proc.json"), "w"), indent=1)
    print("proc goldens:", len(cases), "cases,", len(det), "deterministic; bites", dict(bites))


if __name__ == "__main__":
    main()
