"""Loading of the T5 v1.1 / Flan-T5 fixtures (tests/golden/tiny_v11_*.{npz,json}, made by tests/golden/make_v11_goldens.py) and the
fp32 restatement of the gated feed-forward the kernel tests compare against."""
import json
import math
import os
import types

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("tiny_v11_a", "tiny_v11_b")


def load_v11(name):
    z = np.load(os.path.join(GOLD, f"{name}.npz"))
    meta = json.load(open(os.path.join(GOLD, f"{name}.json")))
    sds = {"swin": {}, "lang": {}, "main": {}}
    grads = {"swin": {}, "main": {}}
    acts = {}
    for k in z.files:
        t = torch.from_numpy(z[k])
        if k.startswith("w."):
            _, m, n = k.split(".", 2)
            sds[m][n] = t
        elif k.startswith("g."):
            _, m, n = k.split(".", 2)
            grads[m][n] = t
        elif k.startswith("act."):
            acts[k[4:]] = t
    inputs = dict(pixel_values=torch.from_numpy(z["pixel_values"]), src_ids=torch.from_numpy(z["src_ids"]), tgt_ids=torch.from_numpy(z["tgt_ids"]))
    return dict(sds=sds, grads=grads, acts=acts, inputs=inputs, loss=float(z["loss"]), meta=meta, greedy_ids=torch.from_numpy(z["greedy_ids"]))


def configs(g):
    """(SwinConfig, lang T5Config, main T5Config) with the main model set to the EFFECTIVE values the reference ran with (recorded in
    the fixture), not to what a library version made of the tie_word_embeddings flag"""
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    meta = g["meta"]
    sw = SwinConfig.from_dict(meta["swin_config"])
    lang = T5Config.from_dict(meta["lang_config"])
    main = T5Config.from_dict(meta["main_config"])
    main.scale_decoder_outputs = bool(meta["effective"]["scaled_logits"])
    main.tie_word_embeddings = bool(meta["effective"]["head_is_tied"])
    return sw, lang, main


def args(train_swin=False, result_dir="/tmp"):
    return types.SimpleNamespace(result_dir=result_dir, language_model_name="-", image_model_name="-", image_model_train=train_swin,
                                 transformer_model_name="-")


def build_v11(name, dtype, train_swin, state_dicts=True):
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_v11(name)
    sds = (g["sds"]["swin"], g["sds"]["lang"], g["sds"]["main"]) if state_dicts else None
    return MyModel(args(train_swin), _configs=configs(g), _state_dicts=sds, dtype=dtype), g


def run(m, g):
    inp = g["inputs"]
    return m({"pixel_values": inp["pixel_values"].cuda()}, {"input_ids": inp["src_ids"].cuda()}, {"input_ids": inp["tgt_ids"].cuda()})


# ---- the gate, restated (HF activations.NewGELUActivation, T5DenseGatedActDense) --------------------------------------------
def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_new_grad(x):
    c = math.sqrt(2.0 / math.pi)
    t = torch.tanh(c * (x + 0.044715 * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * c * (1.0 + 3 * 0.044715 * x * x)


def geglu_ref(a, b, keep_scale):
    """h from the pre-activations a, b [M, F] and keep_scale [M, F] = mask / (1 - p) (ones without dropout)"""
    return gelu_new(a) * b * keep_scale


def geglu_bwd_ref(dh, a, b, keep_scale):
    g = dh * keep_scale
    return g * b * gelu_new_grad(a), g * gelu_new(a)
