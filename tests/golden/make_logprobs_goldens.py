#!/usr/bin/env python3
"""Per-token log-probability goldens from the REFERENCE itself (build container only; CPU).

Runs the reference's own ``MyModel`` (ref/models/model.py:8-42) in fp32 on the weights and inputs of ``tiny_b.npz`` (plain and
EOS-biased, the ``tiny_b.eos_row`` of beam.npz, see make_beam_goldens.py) and ``tiny_v11_a.npz`` (gated feed-forward, untied LM
head; rebuilt from the stored weights and checked against its stored greedy ids) and calls
``.transformer.generate(inputs_embeds=<the reference's concat>, do_sample=False, num_beams=1, max_length=12, output_scores=True,
return_dict_in_generate=True)`` -- HF's greedy loop -- once without processors and once with ``repetition_penalty=1.3,
no_repeat_ngram_size=2, min_length=4``.  Stored per case ``<id>``: the sequences (``<id>.seq`` int64 [rows, L]) and HF's
``compute_transition_scores(sequences, scores, normalize_logits=True)`` (``<id>.logprobs`` f32 [rows, L - 1]: log_softmax of the
processed scores at the chosen token; after a row's EOS it is the log-probability of the forced pad, which the tests ignore).

Guards: every decision up to a row's EOS has a top-2 gap above GAP (no tie the kernel could break differently); the processors
change some sequence; some row of the EOS-biased variant finishes before max_length.

Run:  python tests/golden/make_logprobs_goldens.py      -> logprobs.npz + logprobs.json next to this file
"""
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
from make_v11_goldens import t5_config  # noqa: E402

MAX_LENGTH = 12
GAP = 1e-4
EOS = 1
PROCS = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=4)
MODELS = (("tiny_b", "plain"), ("tiny_b", "eos"), ("tiny_v11_a", "plain"))


def build_dirs_v11(name, z, root):
    """the three checkpoints of a tiny_v11_* fixture from its stored weights (make_v11_goldens.build_dirs without the random init)"""
    from transformers import Swinv2Config, Swinv2Model, T5EncoderModel, T5ForConditionalGeneration
    cfg = json.load(open(os.path.join(HERE, f"{name}.json")))
    swin = Swinv2Model(Swinv2Config(**cfg["swin"]))
    lang = T5EncoderModel(t5_config(cfg["lang"]))
    main = T5ForConditionalGeneration(t5_config(cfg["main"]))
    if main.lm_head.weight.data_ptr() == main.shared.weight.data_ptr():
        main.lm_head.weight = torch.nn.Parameter(torch.randn_like(main.shared.weight))
    main.encoder.embed_tokens.weight = main.shared.weight
    main.decoder.embed_tokens.weight = main.shared.weight
    dirs = {}
    for prefix, m in (("swin", swin), ("lang", lang), ("main", main)):
        sd = {k[len(prefix) + 3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"w.{prefix}.")}
        if prefix != "swin":
            for t in ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight"):
                if t in m.state_dict():
                    sd[t] = sd["shared.weight"]
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all("embed_tokens" in k for k in missing), (missing, unexpected)
        d = os.path.join(root, prefix)
        m.save_pretrained(d)
        dirs[prefix] = d
    assert json.load(open(os.path.join(dirs["main"], "config.json")))["tie_word_embeddings"] is False
    return dirs


def live_mask(seq):
    tok = seq[:, 1:]
    return torch.cumsum(torch.cumsum((tok == EOS).long(), 1), 1) <= 1


def main():
    torch.set_num_threads(4)
    beam = np.load(os.path.join(HERE, "beam.npz"))
    arrays, cases = {}, []
    bites = early = 0
    for name, variant in MODELS:
        z = np.load(os.path.join(HERE, f"{name}.npz"))
        pix, src = torch.from_numpy(z["pixel_values"]), torch.from_numpy(z["src_ids"])
        root = tempfile.mkdtemp(prefix="klab_logprobs_")
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
        seqs = {}
        for pname, kw in (("none", {}), ("procs", PROCS)):
            with torch.no_grad():
                o = model.transformer.generate(inputs_embeds=embeds, do_sample=False, num_beams=1, max_length=MAX_LENGTH,
                                               use_cache=False, output_scores=True, return_dict_in_generate=True, **kw)
            lp = model.transformer.compute_transition_scores(o.sequences, o.scores, normalize_logits=True)
            seq = o.sequences
            assert lp.shape == (seq.shape[0], seq.shape[1] - 1)
            live = live_mask(seq)
            top2 = torch.topk(torch.stack(o.scores, 1).float(), 2, -1)[0]
            assert bool(torch.isfinite(top2[..., 0])[live].all()) and bool(((top2[..., 0] - top2[..., 1]) > GAP)[live].all()), \
                (name, variant, pname, "a decision closer than GAP")
            assert bool(torch.isfinite(lp[live]).all())
            early += int(seq.shape[1] < MAX_LENGTH or bool((~live).any()))
            seqs[pname] = seq
            cid = f"{name}.{variant}.{pname}"
            arrays[cid + ".seq"] = seq.numpy().astype(np.int64)
            arrays[cid + ".logprobs"] = lp.numpy().astype(np.float32)
            cases.append(dict(id=cid, model=name, variant=variant, procs=pname, kwargs=kw, max_length=MAX_LENGTH,
                              rows=int(seq.shape[0]), length=int(seq.shape[1])))
            print(cid, seq.tolist(), flush=True)
        bites += int(seqs["none"].shape != seqs["procs"].shape or not torch.equal(seqs["none"], seqs["procs"]))
    assert bites > 0, "the processors never change a sequence"
    assert early > 0, "no row finishes before max_length"
    np.savez_compressed(os.path.join(HERE, "logprobs.npz"), **arrays)
    json.dump(dict(cases=cases, max_length=MAX_LENGTH, gap=GAP), open(os.path.join(HERE, "logprobs.json"), "w"), indent=1)
    print("logprobs goldens:", len(cases), "cases")


if __name__ == "__main__":
    main()
