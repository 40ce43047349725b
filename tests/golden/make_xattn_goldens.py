#!/usr/bin/env python3
"""Cross-attention-map goldens from the REFERENCE itself (build container only; CPU).

Runs the reference's own ``MyModel`` (ref/models/model.py:8-42) on the weights and inputs of ``tiny_b.npz`` (plain and EOS-biased,
the ``tiny_b.eos_row`` of beam.npz, see make_beam_goldens.py) and ``tiny_v11_a.npz`` (rebuilt from the stored weights as
make_logprobs_goldens.py does), teacher-forced with ``output_attentions=True`` on

(a) the ``<m>.cand`` candidates of force.npz (int64 [B, N, L], as labels are), and
(b) the model's own greedy ids (``transformer.generate(inputs_embeds=..., do_sample=False, num_beams=1, max_length=10,
    use_cache=False)``, stored as ``<m>.greedy_ids`` int64 [B, Lg] with the start token; labels = the ids behind it).

HF returns attention probabilities only from its eager attention, and only when that is chosen at construction
(``_from_config(config, attn_implementation="eager")``; switching a built model does nothing), so ``.transformer`` is rebuilt as an
eager copy with the same state dict.  Before anything is recorded the two are shown to be one model: their state dicts are equal
bit for bit, and their float64 copies give the same logits to 1e-12 (in fp32 the reference's model runs torch's fused attention,
which sums in another order than the eager one: the fp32 logits differ by 1.7e-6, so bit equality cannot be asked there).

Stored per model ``<m>`` = ``<name>.<variant>``, from the float64 copy of that model on the float64 inputs:
``<m>.cand_maps`` f64 [B, N, n_dec_layers, L, Le] and ``<m>.greedy_maps`` f64 [B, n_dec_layers, Lg - 1, Le]: the mean over the heads
of HF's ``cross_attentions`` per layer; position l is the attention that predicts label l.  ``<name>.enc_out`` f64 [B, Le, d]: the
encoder output of that run (one per name: the EOS variant changes a decoder embedding row only, asserted), which tests/xattn_ref.py
restates the decoder over.  xattn.json: per model ``d32`` = max |fp32 run - fp64 run| over both sets of maps, the shapes, and
``image_tokens`` (the Swin tokens come first in Le, the reference's torch.cat order).

Guard: the float64 copy decodes the same greedy ids.

Run:  python tests/golden/make_xattn_goldens.py      -> xattn.npz + xattn.json next to this file
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

MAX_LENGTH = 10
SAME = 1e-12  # float64 logits of the reference's model and of its eager copy (a few hundred ulp of logits of magnitude 5)
MODELS = (("tiny_b", "plain"), ("tiny_b", "eos"), ("tiny_v11_a", "plain"))


def eager_copy(transformer):
    """the same T5ForConditionalGeneration with eager attention (the only one that returns its probabilities)"""
    m = type(transformer)._from_config(copy.deepcopy(transformer.config), attn_implementation="eager")
    if transformer.lm_head.weight.data_ptr() != transformer.shared.weight.data_ptr() and \
            m.lm_head.weight.data_ptr() == m.shared.weight.data_ptr():  # T5 v1.1: an LM head of its own (as build_dirs_v11 unties it)
        m.lm_head.weight = torch.nn.Parameter(torch.empty_like(m.shared.weight))
    m.load_state_dict(transformer.state_dict())
    sa, sb = transformer.state_dict(), m.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa), "the eager copy has other weights"
    return m.eval()


def head_mean_maps(model, embeds, labels):
    """(maps [R, n_dec_layers, L, Le] = mean over the heads of every layer's cross-attention, logits, encoder output)"""
    with torch.no_grad():
        out = model(inputs_embeds=embeds, labels=labels, output_attentions=True)
    assert out.cross_attentions is not None and all(a is not None for a in out.cross_attentions)
    return torch.stack([a.mean(1) for a in out.cross_attentions], 1), out.logits, out.encoder_last_hidden_state


def main():
    torch.set_num_threads(4)
    force = np.load(os.path.join(HERE, "force.npz"))
    arrays, models = {}, []
    for name, variant in MODELS:
        z = np.load(os.path.join(HERE, f"{name}.npz"))
        pix, src = torch.from_numpy(z["pixel_values"]), torch.from_numpy(z["src_ids"])
        root = tempfile.mkdtemp(prefix="klab_xattn_")
        if name.startswith("tiny_v11"):
            model = reference_model(build_dirs_v11(name, z, root))
        else:
            beam = np.load(os.path.join(HERE, "beam.npz"))
            eos_row = torch.from_numpy(beam[f"{name}.eos_row"]) if variant == "eos" else None
            model = reference_model(build_dirs(name, z, root, eos_row))
        shutil.rmtree(root)
        embeds = concat_embeds(model, pix, src)
        B = embeds.shape[0]
        mid = f"{name}.{variant}"
        cand = torch.from_numpy(force[mid + ".cand"])
        _, N, L = cand.shape
        e32 = eager_copy(model.transformer)
        e64 = copy.deepcopy(e32).double()
        with torch.no_grad():
            ids = model.transformer.generate(inputs_embeds=embeds, do_sample=False, num_beams=1, max_length=MAX_LENGTH, use_cache=False)
            again = e64.generate(inputs_embeds=embeds.double(), do_sample=False, num_beams=1, max_length=MAX_LENGTH, use_cache=False)
            assert ids.shape == again.shape and torch.equal(ids, again), (mid, "float64 decodes other greedy ids", ids, again)
            want = copy.deepcopy(model.transformer).double()(inputs_embeds=embeds.double().repeat_interleave(N, 0),
                                                             labels=cand.view(B * N, L)).logits
        d32 = 0.0
        for key, emb, labels in (("cand", embeds.repeat_interleave(N, 0), cand.view(B * N, L)), ("greedy", embeds, ids[:, 1:].contiguous())):
            m32, _, _ = head_mean_maps(e32, emb, labels)
            m64, logits, enc = head_mean_maps(e64, emb.double(), labels)
            if key == "cand":
                gap = float((logits - want).abs().max())
                assert gap <= SAME, (mid, "the eager copy is not the reference's model", gap)
            assert m64.dtype == torch.float64 and float((m64.sum(-1) - 1).abs().max()) < 1e-12
            d32 = max(d32, float((m32.double() - m64).abs().max()))
            arrays[f"{mid}.{key}_maps"] = m64.view(*((B, N) if key == "cand" else (B,)), *m64.shape[1:]).numpy()
            if key == "greedy":
                if name + ".enc_out" in arrays:
                    assert np.array_equal(arrays[name + ".enc_out"], enc.numpy()), (mid, "the variant changes the encoder output")
                arrays[name + ".enc_out"] = enc.numpy().astype(np.float64)
        arrays[mid + ".greedy_ids"] = ids.numpy().astype(np.int64)
        n_img = int(embeds.shape[1] - src.shape[1])
        models.append(dict(id=mid, model=name, variant=variant, B=int(B), d32=d32, n_dec_layers=int(m64.shape[1]), Le=int(embeds.shape[1]),
                           image_tokens=n_img, greedy_length=int(ids.shape[1])))
        print(mid, "d32", d32, "greedy", ids.tolist(), flush=True)
    np.savez_compressed(os.path.join(HERE, "xattn.npz"), **arrays)
    json.dump(dict(models=models, max_length=MAX_LENGTH), open(os.path.join(HERE, "xattn.json"), "w"), indent=1)
    print("xattn goldens:", len(models), "models,", os.path.getsize(os.path.join(HERE, "xattn.npz")), "bytes")


if __name__ == "__main__":
    main()
