#!/usr/bin/env python3
"""Golden vectors for T5 v1.1 / Flan-T5 shaped models (gated gelu_new feed-forward, untied LM head), made by running the
REFERENCE's own ``MyModel`` on CPU exactly as ``make_goldens.py`` does for the v1.0 family.

Writes ``tiny_v11_{a,b}.npz`` / ``.json`` next to this file: inputs, every weight (``lm_head.weight`` separately from
``shared.weight``), the loss, the four captured activations, every gradient of the trainable-Swin run (the frozen run is
asserted to give the same loss), the greedy token ids of ``MyModel(..., return_loss=False)`` with the reference's per-step
top-2 logit margin, and -- because the frozen oracle has no gated layers -- the relative error of the reference model cast to
bf16 against its own fp32 run, per gradient tensor (the bf16 engine test allows twice that).

The JSON records the EFFECTIVE settings the reference ran with (``scaled_logits``, ``head_is_tied``, generation ``max_length``),
measured on the loaded model rather than read from a config flag: the installed ``transformers`` may flip
``tie_word_embeddings`` at construction and again at load.  The tests configure the model under test from these recorded values.

Regenerate (needs the reference checkout and ``transformers``; CPU only, about a minute):

    python tests/golden/make_v11_goldens.py [--only tiny_v11_a]
"""
import argparse
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
from make_goldens import REF, make_inputs  # noqa: E402

V11 = dict(feed_forward_proj="gated-gelu", tie_word_embeddings=False)
MIN_MARGIN = 1e-3  # two orders above the fp32 engine's 1e-5 bound: no position of the greedy comparison may be excluded

CONFIGS = {
    # main gated + untied, language encoder ReLU (mixed); inner_dim 48 != d_model 32; d_ff 192 = 3 x 64 (not a multiple of 128);
    # asymmetric depth (2 encoder layers / 1 decoder layer: HF's generation cache is sized by num_layers, so the decoder is the shallow one)
    "tiny_v11_a": dict(
        swin=dict(image_size=32, patch_size=4, embed_dim=16, depths=[1, 1], num_heads=[1, 2], window_size=4),
        lang=dict(vocab_size=96, d_model=32, d_kv=16, num_heads=2, d_ff=64, num_layers=1, num_decoder_layers=1),
        main=dict(vocab_size=96, d_model=32, d_kv=16, num_heads=3, d_ff=192, num_layers=2, num_decoder_layers=1, **V11),
        B=2, Ls=5, Lt=7, pad_tail=True, seed=53,
    ),
    # both T5s gated, main untied; heads x d_kv = 3 x 8 = 24 against d_model 32 (the 384 / 512 proportion of t5-v1_1-small)
    "tiny_v11_b": dict(
        swin=dict(image_size=32, patch_size=4, embed_dim=16, depths=[1, 1], num_heads=[1, 2], window_size=4),
        lang=dict(vocab_size=128, d_model=32, d_kv=8, num_heads=3, d_ff=64, num_layers=1, num_decoder_layers=1,
                  feed_forward_proj="gated-gelu"),
        main=dict(vocab_size=128, d_model=32, d_kv=8, num_heads=3, d_ff=128, num_layers=2, num_decoder_layers=2, **V11),
        B=2, Ls=6, Lt=9, pad_tail=True, seed=67,
    ),
}


def t5_config(kw):
    from transformers import T5Config
    kw = dict(kw)
    untie = kw.pop("tie_word_embeddings", True) is False
    c = T5Config(**kw, decoder_start_token_id=0)
    if untie:  # the constructor argument may come back True: set the attribute, and check what will be written
        c.tie_word_embeddings = False
        assert c.to_dict()["tie_word_embeddings"] is False
    return c


def build_dirs(cfg, root):
    from transformers import Swinv2Config, Swinv2Model, T5EncoderModel, T5ForConditionalGeneration
    torch.manual_seed(cfg["seed"])
    swin = Swinv2Model(Swinv2Config(**cfg["swin"]))
    lang = T5EncoderModel(t5_config(cfg["lang"]))
    main = T5ForConditionalGeneration(t5_config(cfg["main"]))
    if main.lm_head.weight.data_ptr() == main.shared.weight.data_ptr():  # construction tied them after all: give the head its own tensor
        main.lm_head.weight = torch.nn.Parameter(torch.randn_like(main.shared.weight))
    # an untied config leaves the two embed_tokens tables as tensors of their own as well; every published v1.1 / Flan-T5 checkpoint
    # holds shared.weight in them, so make them one parameter again (perturbed once, saved with equal values)
    main.encoder.embed_tokens.weight = main.shared.weight
    main.decoder.embed_tokens.weight = main.shared.weight
    # perturb every tensor as make_goldens.build_dirs does; lm_head.weight is a parameter of its own here, so it gets its own noise
    g = torch.Generator().manual_seed(cfg["seed"] + 1)
    with torch.no_grad():
        for m in (swin, lang, main):
            for n, p in m.named_parameters():
                p.add_(torch.randn(p.shape, generator=g) * 0.05 * (p.abs().mean() + 0.02))
    assert "lm_head.weight" in dict(main.named_parameters())
    dirs = {}
    for name, m in (("swin", swin), ("lang", lang), ("main", main)):
        d = os.path.join(root, name)
        m.save_pretrained(d)
        dirs[name] = d
    assert json.load(open(os.path.join(dirs["main"], "config.json")))["tie_word_embeddings"] is False
    return dirs


def load_reference(dirs, train_swin):
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    from models.model import MyModel  # the reference's own class
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name=dirs["lang"], image_model_name=dirs["swin"],
                                 image_model_train=train_swin, transformer_model_name=dirs["main"])
    model = MyModel(args)
    model.transformer.eval()
    return model


def run_reference(cfg, dirs, train_swin, dtype=torch.float32):
    model = load_reference(dirs, train_swin)
    if dtype != torch.float32:
        model = model.to(dtype)
    pix, src, tgt = make_inputs(dict(cfg, t5=cfg["main"]))
    pix = pix.to(dtype)
    caps, head_in = {}, []

    def cap(name):
        def hook(_m, _i, out):
            caps[name] = out.last_hidden_state.detach().clone() if hasattr(out, "last_hidden_state") else out
        return hook

    model.image_model.register_forward_hook(cap("image_embeddings"))
    model.language_model.register_forward_hook(cap("language_embeddings"))
    model.transformer.encoder.register_forward_hook(cap("encoder_out"))
    model.transformer.decoder.register_forward_hook(cap("decoder_out"))
    h = model.transformer.lm_head.register_forward_hook(lambda _m, i, _o: head_in.append(i[0].detach().clone()))
    loss = model({"pixel_values": pix}, {"input_ids": src}, {"input_ids": tgt})
    loss.backward()
    h.remove()
    tr = model.transformer
    eff = dict(
        # what the arithmetic did, not what a flag says: was the decoder output scaled in front of the head, is the head shared.weight
        scaled_logits=not torch.equal(head_in[0], caps["decoder_out"]),
        head_is_tied=bool(tr.lm_head.weight.data_ptr() == tr.shared.weight.data_ptr() or torch.equal(tr.lm_head.weight, tr.shared.weight)),
    )
    if eff["scaled_logits"]:
        assert torch.allclose(head_in[0], caps["decoder_out"] * tr.config.d_model ** -0.5)
    out = dict(pixel_values=pix, src_ids=src, tgt_ids=tgt, loss=loss.detach())
    for k, v in caps.items():
        out["act." + k] = v
    for prefix, m in (("main.", tr), ("swin.", model.image_model), ("lang.", model.language_model)):
        sd = m.state_dict()
        for n, p in sd.items():
            if n in ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight"):
                assert torch.equal(p, sd["shared.weight"])
                continue
            out["w." + prefix + n] = p.detach()
        for n, p in m.named_parameters():
            if p.grad is None:
                continue
            if n in ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight"):  # loaded as a tensor of its own with shared.weight's
                n = "shared.weight"                                                  # values: its gradient is the embedding table's
            key = "g." + prefix + n
            out[key] = out[key] + p.grad.detach() if key in out else p.grad.detach().clone()
    return out, eff, model


def greedy(model, cfg):
    """MyModel(..., return_loss=False) with the lm_head's outputs captured: ids, and per step the smallest top-2 margin over the rows"""
    pix, src, _tgt = make_inputs(dict(cfg, t5=cfg["main"]))
    steps = []
    h = model.transformer.lm_head.register_forward_hook(lambda _m, _i, o: steps.append(o.detach()[:, -1].float().clone()))
    with torch.no_grad():
        ids = model({"pixel_values": pix}, {"input_ids": src}, return_loss=False)
    h.remove()
    margins = []
    for lg in steps[:ids.shape[1] - 1]:
        top = lg.topk(2, dim=-1).values
        margins.append(float((top[:, 0] - top[:, 1]).min()))
    # the length limit in effect: the generation config's when it has one, otherwise what the library's default made of it -- the
    # observed length, which is that limit when some row was still open at the end, and no limit at all when every row ended early
    gl = model.transformer.generation_config.max_length or ids.shape[1]
    assert ids.shape[1] <= gl
    return ids, margins, int(gl)


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    torch.set_num_threads(4)
    for name, cfg in CONFIGS.items():
        if a.only and a.only != name:
            continue
        root = tempfile.mkdtemp(prefix="klab_gold_")
        dirs = build_dirs(cfg, root)
        out, eff, model = run_reference(cfg, dirs, train_swin=True)
        out_frozen, eff_f, _ = run_reference(cfg, dirs, train_swin=False)
        assert torch.equal(out["loss"], out_frozen["loss"]) and eff == eff_f
        assert not any(k.startswith("g.swin.") for k in out_frozen)
        for k in out_frozen:
            if k.startswith("g.main."):
                assert torch.equal(out[k], out_frozen[k]), k
        assert not eff["head_is_tied"], "the reference tied the LM head: the fixture would not pin the untied arithmetic"
        assert not torch.equal(out["w.main.lm_head.weight"], out["w.main.shared.weight"])
        ids, margins, gen_len = greedy(model, cfg)
        assert min(margins) >= MIN_MARGIN, (name, "smallest top-2 margin", min(margins), "pick another seed")
        out["greedy_ids"] = ids
        # the reference's own bf16 error: the same model and inputs cast to bf16 on CPU, against the fp32 run above
        out16, _e, _m = run_reference(cfg, dirs, train_swin=True, dtype=torch.bfloat16)
        err = {k: rel_l2(out16[k].float(), out[k]) for k in out if k.startswith("g.")}
        gk = sorted(err)
        err["all"] = rel_l2(torch.cat([out16[k].float().flatten() for k in gk]), torch.cat([out[k].flatten() for k in gk]))
        err["loss"] = abs(float(out16["loss"]) - float(out["loss"])) / abs(float(out["loss"]))
        np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **{k: v.numpy() for k, v in out.items()})
        cfg_json = {k: v for k, v in cfg.items()}
        cfg_json["swin_config"] = json.load(open(os.path.join(dirs["swin"], "config.json")))
        cfg_json["lang_config"] = json.load(open(os.path.join(dirs["lang"], "config.json")))
        cfg_json["main_config"] = json.load(open(os.path.join(dirs["main"], "config.json")))
        cfg_json["effective"] = dict(eff, generation_max_length=gen_len)
        cfg_json["greedy_margins"] = margins
        cfg_json["bf16_reference_error"] = err
        json.dump(cfg_json, open(os.path.join(HERE, f"{name}.json"), "w"), indent=1, sort_keys=True)
        print(name, "loss", float(out["loss"]), "tensors", len(out), "effective", cfg_json["effective"], "min margin", min(margins),
              "greedy length", ids.shape[1], "bf16 error overall", err["all"], "bytes", os.path.getsize(os.path.join(HERE, f"{name}.npz")))
        shutil.rmtree(root)


if __name__ == "__main__":
    main()
