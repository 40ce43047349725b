#!/usr/bin/env python3
"""Constrained-decoding goldens from the REFERENCE itself (build container only; CPU).

Runs the reference's own ``MyModel`` on the weights and inputs of ``tiny_a.npz`` / ``tiny_b.npz``, plain and EOS-biased (the
``<model>.eos_row`` of beam.npz, see make_beam_goldens.py), and calls ``.transformer.generate(inputs_embeds=<the reference's
concat>, prefix_allowed_tokens_fn=<callback>, ...)``.  The callback is a dict trie (tests/constrain_ref.py): the children of the
node the row stands on, ``[eos]`` at a leaf and off the trie (where HF itself would raise), image = ``batch_id``, which HF
computes as ``row // num_beams``.

Phrase sets (``sets`` in constrain.json) are built per model by seeded random walks over ids >= 2: sizes 3, 17 and 200, lengths
1 to 6 with shared prefixes, one phrase a prefix of another, a one-token phrase.  Cases: every set alone and (greedy, sample)
behind a decoder prompt, the 17-phrase sets also with ``no_repeat_ngram_size``, ``repetition_penalty`` and ``min_new_tokens``,
plus a two-set case with alternating ``constraint_set``; sampling cases from tiny_b only (the suite stays quick):
  greedy   -- the sequences (``<id>.seq``); kept only when an fp64 rerun gives the same sequences and every live step's processed
              top-2 gap exceeds GAP (never an all -inf row);
  beam     -- num_beams 2 and 4: the sequences and ``sequences_scores``; kept under the fp64 rerun and score-gap filter of
              make_proc_goldens.py and only when every returned score is finite;
  sample   -- ``torch.manual_seed(<case index>)``, per generated step the kept set of the processed + warped scores
              (``<id>.kept``, packed bits) and the sampled sequences (teacher-forcing inputs for the tests, never an expected
              output); a case whose settings leave some row without a finite score (HF raises) is dropped.

Also stored: HF's ``PrefixConstrainedLogitsProcessor`` itself on random scores and histories (on the trie, at leaves, past EOS,
off the trie) at num_beams 1 and 3 (``pin_x``, ``pin_hist`` padded with -1, ``pin_out``; settings in ``pin``), which pin the tests'
torch restatement.

Guards: at least 30 deterministic and 15 sample cases remain; for every phrase-set size some case differs from the unconstrained
call.

Run:  python tests/golden/make_constrain_goldens.py      -> constrain.npz + constrain.json next to this file
"""
import collections
import importlib.util
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

# tests/constrain_ref.py by its path: the repository root must stay off sys.path, where its `models` package would shadow the reference's
_spec = importlib.util.spec_from_file_location("constrain_ref", os.path.join(os.path.dirname(HERE), "constrain_ref.py"))
_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ref)
DictTrie, callback, random_phrases = _ref.DictTrie, _ref.callback, _ref.random_phrases

MODELS = ("tiny_a", "tiny_b")
MAX_LENGTH = 10
GAP = 1e-4
EOS = 1
SIZES = (3, 17, 200)
GRID_SIZE = 17            # the processors are combined with the sets of this size; the other sets run alone and with a prompt
SAMPLE_MODEL = "tiny_b"   # sampling cases (each costs the tests a teacher-forced forward per step) come from one model
PIN_V, PIN_H, PIN_N, PIN_ROWS = 48, 9, 120, 6


def phrase_set(rng, n, vocab):
    """n phrases with the shapes the issue names: a one-token phrase, a phrase that is a prefix of another"""
    ps = random_phrases(rng, n, vocab)
    if not any(len(p) == 1 for p in ps):
        ps[0] = [ps[1][0]] if n > 1 and [ps[1][0]] not in ps else ps[0][:1]
    longest = max(ps, key=len)
    if len(longest) > 1 and longest[:-1] not in ps:
        ps[-1] = longest[:-1]
    out = []
    for p in ps:
        if p not in out:
            out.append(p)
    return out


def proc_grid():
    return collections.OrderedDict([
        ("alone", {}),
        ("ngram2", dict(no_repeat_ngram_size=2)),
        ("rep", dict(repetition_penalty=1.3)),
        ("minnew", dict(min_new_tokens=2)),
    ])


def pin_goldens(arrays):
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor
    rng = random.Random(11)
    g = torch.Generator().manual_seed(11)
    sets = [phrase_set(rng, 12, PIN_V), phrase_set(rng, 5, PIN_V)]
    trie = DictTrie(sets, EOS)
    xs, hs, outs, meta = [], [], [], []
    for i in range(PIN_N):
        nb = (1, 3)[i % 2]
        which = [rng.randrange(2) for _ in range(PIN_ROWS // nb)]
        L = rng.randint(1, PIN_H)
        hist = torch.zeros(PIN_ROWS, L, dtype=torch.int64)
        for r in range(PIN_ROWS):
            kind = rng.random()
            p = rng.choice(sets[which[r // nb]])
            if kind < 0.6:    # on the trie, possibly through EOS and into the pads behind it
                body = (p + [EOS] + [0] * PIN_H)[:L - 1]
            elif kind < 0.8:  # leaves the trie somewhere
                body = (p[:rng.randint(0, len(p))] + [rng.randrange(2, PIN_V) for _ in range(PIN_H)])[:L - 1]
            else:
                body = [rng.randrange(0, PIN_V) for _ in range(L - 1)]
            hist[r, 1:] = torch.tensor(body, dtype=torch.int64)
        x = torch.randn(PIN_ROWS, PIN_V, generator=g) * 3.0
        out = PrefixConstrainedLogitsProcessor(callback(trie, which, nb), nb)(hist, x.clone())
        hp = torch.full((PIN_ROWS, PIN_H), -1, dtype=torch.int64)
        hp[:, :L] = hist
        xs.append(x.numpy()); hs.append(hp.numpy()); outs.append(out.numpy())
        meta.append(dict(cur_len=L, num_beams=nb, sets=which))
    arrays["pin_x"] = np.stack(xs).astype(np.float32)
    arrays["pin_hist"] = np.stack(hs)
    arrays["pin_out"] = np.stack(outs).astype(np.float32)
    return dict(cases=meta, phrase_sets=sets)


def gen(model, embeds, mode, kw, fn, prompt=None, **extra):
    common = dict(inputs_embeds=embeds, max_length=MAX_LENGTH, use_cache=False, output_scores=True, return_dict_in_generate=True)
    if fn is not None:
        common["prefix_allowed_tokens_fn"] = fn
    if prompt is not None:
        common["decoder_input_ids"] = prompt
    with torch.no_grad():
        if mode == "greedy":
            o = model.transformer.generate(do_sample=False, num_beams=1, **common, **kw)
            return o.sequences, torch.stack(o.scores, 1)
        if mode == "beam":
            o = model.transformer.generate(do_sample=False, **common, **extra, **kw)
            return o.sequences, o.sequences_scores.float()
        o = model.transformer.generate(do_sample=True, **common, **extra, **kw)
        return o.sequences, torch.stack(o.scores, 1)


def live_mask(tok):
    return torch.cumsum(torch.cumsum((tok == EOS).long(), 1), 1) <= 1


def main():
    torch.set_num_threads(4)
    beam = np.load(os.path.join(HERE, "beam.npz"))
    arrays, cases, sets_json = {}, [], {}
    pin = pin_goldens(arrays)
    bites = collections.Counter()
    sample_idx = 0
    for name in MODELS:
        z = np.load(os.path.join(HERE, f"{name}.npz"))
        pix, src = torch.from_numpy(z["pixel_values"]), torch.from_numpy(z["src_ids"])
        B = src.shape[0]
        rng = random.Random(sum(map(ord, name)))
        for variant in ("plain", "eos"):
            root = tempfile.mkdtemp(prefix="klab_constrain_")
            eos_row = torch.from_numpy(beam[f"{name}.eos_row"]) if variant == "eos" else None
            model = reference_model(build_dirs(name, z, root, eos_row))
            embeds = concat_embeds(model, pix, src)
            model64 = reference_model(build_dirs(name, z, root, eos_row)).double()
            embeds64 = concat_embeds(model64, pix.double(), src)
            shutil.rmtree(root)
            vocab = int(model.transformer.config.vocab_size)
            if variant == "plain":
                for n in SIZES:
                    sets_json[f"{name}.s{n}"] = phrase_set(rng, n, vocab)
                prompt = torch.tensor([[rng.randrange(2, vocab), rng.randrange(2, vocab)] for _ in range(B)], dtype=torch.int64)
                arrays[f"{name}.prompt"] = prompt.numpy()
            # (set names, the set of every image)
            layouts = [((f"{name}.s{n}",), [0] * B, n) for n in SIZES] + [((f"{name}.s17", f"{name}.s200"), [b % 2 for b in range(B)], "two")]
            modes = [("greedy", {}), ("beam", dict(num_beams=2)), ("beam", dict(num_beams=4)),
                     ("sample", dict(top_k=0)), ("sample", dict(top_k=5, temperature=0.7))]
            for names, which, size in layouts:
                trie = DictTrie([sets_json[s] for s in names], EOS)
                for mode, extra in modes:
                    nb = extra.get("num_beams", 1)
                    if mode == "sample" and name != SAMPLE_MODEL:
                        continue
                    variants = list(proc_grid().items()) if size == GRID_SIZE else [("alone", {})]
                    if mode != "beam":
                        variants.append(("prompt", {}))
                    free = {}
                    for pname, kw in variants:
                        pr = prompt if pname == "prompt" else None
                        fn = callback(trie, which, nb, skip=1 + (pr.shape[1] if pr is not None else 0))
                        tag = ".".join(f"{k}{v}" for k, v in extra.items())
                        cid = ".".join(x for x in (name, variant, f"s{size}", mode, tag, pname) if x)
                        cs = dict(id=cid, model=name, variant=variant, mode=mode, procs=pname, kwargs=kw, max_length=MAX_LENGTH,
                                  vocab=vocab, sets=list(names), constraint_set=which, size=str(size), prompt=pr is not None, **extra)
                        if mode == "sample":
                            torch.manual_seed(sample_idx)
                            sample_idx += 1
                            try:
                                seq, sc = gen(model, embeds, mode, kw, fn, pr, **extra)
                            except (RuntimeError, ValueError):  # a row without a finite score
                                continue
                            arrays[cid + ".seq"] = seq.numpy().astype(np.int64)
                            arrays[cid + ".kept"] = np.packbits((sc > -float("inf")).numpy(), axis=-1)
                            cases.append(cs)
                            continue
                        seq, sc = gen(model, embeds, mode, kw, fn, pr, **extra)
                        key = (pname == "prompt")
                        if key not in free:
                            free[key] = gen(model, embeds, mode, {}, None, pr, **extra)[0]
                        if seq.shape != free[key].shape or not torch.equal(seq, free[key]):
                            bites[str(size)] += 1
                        seq64, sc64 = gen(model64, embeds64, mode, kw, fn, pr, **extra)
                        if seq.shape != seq64.shape or not torch.equal(seq, seq64):
                            continue
                        if mode == "greedy":
                            top2 = torch.topk(sc.float(), 2, -1)[0]
                            live = live_mask(seq[:, seq.shape[1] - sc.shape[1]:])
                            if not bool(torch.isfinite(top2[..., 0])[live].all()) or not bool(((top2[..., 0] - top2[..., 1]) > GAP)[live].all()):
                                continue
                        else:
                            if not bool(torch.isfinite(sc).all()) or not torch.allclose(sc.double(), sc64.double(), atol=1e-4, rtol=0):
                                continue
                            arrays[cid + ".scores"] = sc.numpy().astype(np.float32)
                        arrays[cid + ".seq"] = seq.numpy().astype(np.int64)
                        cases.append(cs)
            print(name, variant, "cases so far", len(cases), flush=True)
    det = [c for c in cases if c["mode"] != "sample"]
    for size in list(map(str, SIZES)) + ["two"]:
        assert bites[size] > 0, f"phrase sets of size {size} never change an output"
    assert len(det) >= 30, f"only {len(det)} deterministic cases survive the filters"
    assert len(cases) - len(det) >= 15, f"only {len(cases) - len(det)} sample cases remain"
    np.savez_compressed(os.path.join(HERE, "constrain.npz"), **arrays)
    json.dump(dict(cases=cases, sets=sets_json, pin=pin, pin_shape=[PIN_N, PIN_ROWS, PIN_V, PIN_H], max_length=MAX_LENGTH,
                   bites=dict(bites)), open(os.path.join(HERE, "constrain.json"), "w"), indent=1)
    print("constrain goldens:", len(cases), "cases,", len(det), "deterministic; bites", dict(bites))


if __name__ == "__main__":
    main()
