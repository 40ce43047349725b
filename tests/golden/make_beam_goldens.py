#!/usr/bin/env python3
"""Beam-search goldens from the REFERENCE itself (build container only; CPU).

Runs the reference's own ``MyModel`` (ref/models/model.py:8-42) on the weights and inputs already stored in
``tiny_a.npz`` / ``tiny_b.npz`` / ``tiny_c.npz`` and calls ``.transformer.generate(inputs_embeds=<the reference's concat>,
num_beams=...)`` -- HF's ``_beam_search`` -- over a grid of num_beams, length_penalty, early_stopping, num_return_sequences
and max_length.  Random-init tiny models almost never emit EOS (id 1), so every model also runs in an EOS-biased variant
whose ``shared.weight[1]`` is replaced by a row along the mean decoder-output direction (stored as ``<variant>.eos_row``).
``use_cache=False``: HF 5.15's DynamicCache raises IndexError when num_decoder_layers != num_layers (tiny_b); without the
cache the result is the same mathematically.

Guards (a fixture too weak to test anything fails here): some case returns hypotheses of one sample that finish at different
lengths; some case differs between early_stopping=True and False; every kept case gives the same sequences under an fp64 rerun
and its consecutive returned scores differ by more than 1e-4 (other cases are dropped); at least 12 cases remain.

Run:  python tests/golden/make_beam_goldens.py      -> beam.npz + beam.json next to this file
"""
import itertools
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import REF  # noqa: E402

MODELS = ("tiny_a", "tiny_b", "tiny_c")
NUM_BEAMS = (2, 4)
LENGTH_PENALTY = (1.0, 0.0, 2.0)
EARLY_STOPPING = (False, True, "never")
MAX_LENGTHS = (7, 12)
EOS_SCALE = 0.8  # |eos row| = EOS_SCALE * mean row norm of shared.weight


def build_dirs(name, z, root, eos_row=None):
    from transformers import Swinv2Config, Swinv2Model, T5Config, T5EncoderModel, T5ForConditionalGeneration
    cfg = json.load(open(os.path.join(HERE, f"{name}.json")))
    swin = Swinv2Model(Swinv2Config(**cfg["swin"]))
    # one config object each: T5EncoderModel clears is_encoder_decoder on the config it is given
    lang = T5EncoderModel(T5Config(**cfg["t5"], decoder_start_token_id=0))
    main = T5ForConditionalGeneration(T5Config(**cfg["t5"], decoder_start_token_id=0))
    assert main.config.is_encoder_decoder
    dirs = {}
    for prefix, m in (("swin", swin), ("lang", lang), ("main", main)):
        sd = {k[len(prefix) + 3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"w.{prefix}.")}
        if prefix != "swin":
            if eos_row is not None and prefix == "main":
                sd["shared.weight"] = sd["shared.weight"].clone()
                sd["shared.weight"][1] = eos_row
            for t in ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight", "lm_head.weight"):
                if t in m.state_dict():
                    sd[t] = sd["shared.weight"]
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all("embed_tokens" in k or k == "lm_head.weight" for k in missing), (missing, unexpected)
        d = os.path.join(root, prefix)
        m.save_pretrained(d)
        dirs[prefix] = d
    return dirs


def reference_model(dirs):
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    from models.model import MyModel  # the reference's own class
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name=dirs["lang"], image_model_name=dirs["swin"],
                                 image_model_train=False, transformer_model_name=dirs["main"])
    model = MyModel(args)
    model.eval()
    return model


def concat_embeds(model, pix, src):
    """the reference's torch.cat((image_embeddings, language_embeddings), dim=1) (ref/models/model.py:20-23)"""
    caps = {}
    orig = model.transformer.generate

    def grab(*a, **k):
        caps["embeds"] = k["inputs_embeds"]
        return None
    model.transformer.generate = grab
    try:
        with torch.no_grad():
            model({"pixel_values": pix}, {"input_ids": src}, return_loss=False)
    finally:
        model.transformer.generate = orig
    return caps["embeds"]


def run_case(model, embeds, nb, lp, es, nrs, ml):
    with torch.no_grad():
        out = model.transformer.generate(inputs_embeds=embeds, num_beams=nb, length_penalty=lp, early_stopping=es,
                                         num_return_sequences=nrs, max_length=ml, use_cache=False, do_sample=False,
                                         output_scores=True, return_dict_in_generate=True)
    return out.sequences, out.sequences_scores.float()


def eos_row_for(model, z):
    """a row along the mean decoder-output direction (the LM head's input), EOS_SCALE x the mean row norm"""
    shared = torch.from_numpy(z["w.main.shared.weight"])
    u = torch.from_numpy(z["act.decoder_out"]).reshape(-1, shared.shape[1]).mean(0)
    return u / u.norm() * EOS_SCALE * shared.norm(dim=1).mean()


def main():
    torch.set_num_threads(4)
    arrays, cases = {}, []
    saw_len_diff = saw_es_diff = False
    for name in MODELS:
        z = np.load(os.path.join(HERE, f"{name}.npz"))
        pix, src = torch.from_numpy(z["pixel_values"]), torch.from_numpy(z["src_ids"])
        for variant in ("plain", "eos"):
            root = tempfile.mkdtemp(prefix="klab_beam_")
            eos_row = None
            if variant == "eos":
                eos_row = eos_row_for(None, z)
                arrays[f"{name}.eos_row"] = eos_row.numpy()
            model = reference_model(build_dirs(name, z, root, eos_row))
            embeds = concat_embeds(model, pix, src)
            model64 = reference_model(build_dirs(name, z, root, eos_row)).double()
            embeds64 = concat_embeds(model64, pix.double(), src)
            shutil.rmtree(root)
            by_es = {}
            for nb, lp, es, ml in itertools.product(NUM_BEAMS, LENGTH_PENALTY, EARLY_STOPPING, MAX_LENGTHS):
                for nrs in (1, nb):
                    seq, sc = run_case(model, embeds, nb, lp, es, nrs, ml)
                    seq64, _ = run_case(model64, embeds64, nb, lp, es, nrs, ml)
                    by_es.setdefault((nb, lp, ml, nrs), {})[es] = seq
                    B = src.shape[0]
                    gen_len = (seq[:, 1:] != 1).cumprod(1).sum(1) + (seq[:, 1:] == 1).any(1).long()  # tokens up to the first EOS
                    if nrs > 1 and any(len(set(gen_len[b * nrs:(b + 1) * nrs].tolist())) > 1 for b in range(B)):
                        saw_len_diff = True
                    gaps_ok = all(float((sc[b * nrs + i] - sc[b * nrs + i + 1]).abs()) > 1e-4
                                  for b in range(B) for i in range(nrs - 1))
                    if not torch.equal(seq, seq64) or not gaps_ok:
                        continue
                    cid = f"{name}.{variant}.k{nb}.lp{lp}.es{es}.n{nrs}.ml{ml}"
                    arrays[cid + ".seq"] = seq.numpy().astype(np.int64)
                    arrays[cid + ".scores"] = sc.numpy().astype(np.float32)
                    cases.append(dict(id=cid, model=name, variant=variant, num_beams=nb, length_penalty=lp, early_stopping=es,
                                      num_return_sequences=nrs, max_length=ml))
            for d in by_es.values():
                if not torch.equal(d[True], d[False]) if d[True].shape == d[False].shape else True:
                    saw_es_diff = True
            print(name, variant, "cases kept so far", len(cases), flush=True)
    assert saw_len_diff, "no case returns hypotheses of one sample that finish at different lengths"
    assert saw_es_diff, "early_stopping=True and False never differ"
    assert len(cases) >= 12, f"only {len(cases)} cases survive the fp64 / score-gap filter"
    np.savez_compressed(os.path.join(HERE, "beam.npz"), **arrays)
    json.dump(dict(cases=cases, eos_scale=EOS_SCALE), open(os.path.join(HERE, "beam.json"), "w"), indent=1)
    print("beam goldens:", len(cases), "cases")


if __name__ == "__main__":
    main()
