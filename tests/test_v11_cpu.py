"""T5 v1.1 / Flan-T5 support, the part that needs no GPU: configuration parsing, the C struct mirrors, the parameter schema of the
two fixtures (tests/golden/tiny_v11_*.npz; regenerate with tests/golden/make_v11_goldens.py) and the loading rules of an untied head."""
import ctypes as C
import os

import pytest
import torch

from tests.v11_helpers import GOLD, NAMES, args, build_v11, configs, load_v11

HF_ALIASES = {"encoder.embed_tokens.weight", "decoder.embed_tokens.weight"}  # of shared.weight, in an untied T5ForConditionalGeneration


def test_struct_mirrors_have_the_c_sizes():
    from klab_multimodalmodel_amd import engine as E
    lib = E.lib()
    assert lib.klab_sizeof_t5_cfg() == C.sizeof(E.CT5Cfg)
    assert lib.klab_sizeof_model_cfg() == C.sizeof(E.CModelCfg)
    names = [f[0] for f in E.CT5Cfg._fields_]
    assert names[-2:] == ["ffn_gated", "tie_lm_head"] and names[-3] == "scale_decoder_outputs"  # appended, nothing moved


def test_flags_reach_the_c_config():
    from klab_multimodalmodel_amd.engine import T5Config, _c_t5
    v10 = _c_t5(T5Config.from_dict({"d_model": 64}))
    assert (v10.ffn_gated, v10.tie_lm_head, v10.scale_decoder_outputs) == (0, 1, 1)
    v11 = _c_t5(T5Config.from_dict({"d_model": 64, "feed_forward_proj": "gated-gelu", "tie_word_embeddings": False}))
    assert (v11.ffn_gated, v11.tie_lm_head, v11.scale_decoder_outputs) == (1, 0, 0)  # HF's rule: untied => unscaled
    mixed = _c_t5(T5Config.from_dict({"d_model": 64, "feed_forward_proj": "gated-gelu"}))
    assert (mixed.ffn_gated, mixed.tie_lm_head, mixed.scale_decoder_outputs) == (1, 1, 1)


@pytest.mark.parametrize("proj", ["gated-silu", "gelu", "gated-relu", "silu"])
def test_other_feed_forwards_still_raise(proj):
    from klab_multimodalmodel_amd.engine import T5Config, _c_t5
    with pytest.raises(NotImplementedError, match="feed_forward_proj"):
        _c_t5(T5Config.from_dict({"feed_forward_proj": proj}))


def test_fp8_with_gated_layers_raises():
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_v11("tiny_v11_a")
    with pytest.raises(NotImplementedError, match="fp8"):
        MyModel(args(), _configs=configs(g), dtype="fp8")
    sw, lang, main = configs(g)
    lang.feed_forward_proj = main.feed_forward_proj = "relu"
    MyModel(args(), _configs=(sw, lang, main), dtype="fp8")  # ... and only with them


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_what_the_issue_asks_for(name):
    g = load_v11(name)
    meta = g["meta"]
    assert meta["main_config"]["feed_forward_proj"] == "gated-gelu" and meta["main_config"]["tie_word_embeddings"] is False
    assert meta["effective"]["head_is_tied"] is False
    assert not torch.equal(g["sds"]["main"]["lm_head.weight"], g["sds"]["main"]["shared.weight"])
    assert min(meta["greedy_margins"]) >= 1e-3  # no position of the greedy comparison needs excluding
    assert g["greedy_ids"].shape[1] <= meta["effective"]["generation_max_length"]
    assert "g.main.lm_head.weight" in meta["bf16_reference_error"] and "g.main.shared.weight" in meta["bf16_reference_error"]
    mc = meta["main_config"]
    assert mc["num_heads"] * mc["d_kv"] != mc["d_model"]
    if name == "tiny_v11_a":
        assert meta["lang_config"]["feed_forward_proj"] == "relu" and mc["d_ff"] % 64 == 0 and mc["d_ff"] % 128 != 0
        assert mc["num_layers"] != mc["num_decoder_layers"]
    else:
        assert meta["lang_config"]["feed_forward_proj"] == "gated-gelu"
        assert 4 * mc["num_heads"] * mc["d_kv"] == 3 * mc["d_model"]  # the 384 / 512 proportion of t5-v1_1-small
    for f in (f"{name}.npz", f"{name}.json"):
        assert os.path.getsize(os.path.join(GOLD, f)) < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_schema_equals_the_references(name):
    m, g = build_v11(name, "fp32", False)
    for tree, key in ((m.transformer, "main"), (m.language_model, "lang"), (m.image_model, "swin")):
        own = {k: tuple(v.shape) for k, v in tree.state_dict().items()}
        ref = {k: tuple(v.shape) for k, v in g["sds"][key].items()}
        if key == "main":
            assert "lm_head.weight" in ref and any(".wi_0." in k for k in ref) and not any(k.endswith(".wi.weight") for k in ref)
            ref.update({a: ref["shared.weight"] for a in HF_ALIASES})
        elif key == "lang":
            ref["encoder.embed_tokens.weight"] = ref["shared.weight"]
        ref = {k: v for k, v in ref.items() if k in own or not k.endswith(("relative_position_index", "relative_coords_table"))}
        assert own == ref, (key, sorted(set(own) ^ set(ref)))
    sd = m.transformer.state_dict()
    assert sd["lm_head.weight"].data_ptr() != sd["shared.weight"].data_ptr()
    assert sd["decoder.embed_tokens.weight"].data_ptr() == sd["shared.weight"].data_ptr()
    for k, v in g["sds"]["main"].items():
        assert torch.equal(sd[k], v), k
    names = [n for n, _p in m.transformer.named_parameters()]
    assert "lm_head.weight" in names and len(names) == len(g["sds"]["main"])  # each tensor once: what an optimizer sees


def test_untied_model_demands_its_lm_head():
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_v11("tiny_v11_a")
    sd = dict(g["sds"]["main"])
    del sd["lm_head.weight"]
    with pytest.raises(RuntimeError, match=r"Missing key\(s\) in state_dict.*lm_head.weight"):
        MyModel(args(), _configs=configs(g), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], sd), dtype="fp32")
    # a tied model does not: the same state dict loads into the tied variant of the configuration
    sw, lang, main = configs(g)
    main.tie_word_embeddings = True
    m = MyModel(args(), _configs=(sw, lang, main), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], sd), dtype="fp32")
    assert m.transformer.state_dict()["lm_head.weight"].data_ptr() == m.transformer.state_dict()["shared.weight"].data_ptr()


def test_random_init_gives_the_untied_head_hf_statistics():
    m, g = build_v11("tiny_v11_b", "fp32", False, state_dicts=False)
    sd = m.transformer.state_dict()
    d = m.main_cfg.d_model
    assert abs(float(sd["lm_head.weight"].std()) - 1.0) < 0.1 and not torch.equal(sd["lm_head.weight"], sd["shared.weight"])
    for k in ("encoder.block.0.layer.1.DenseReluDense.wi_0.weight", "encoder.block.0.layer.1.DenseReluDense.wi_1.weight"):
        assert abs(float(sd[k].std()) * d ** 0.5 - 1.0) < 0.1, k


def test_known_v11_names_build_with_random_init(monkeypatch):
    from klab_multimodalmodel_amd import hf_io
    monkeypatch.setenv("KLAB_ALLOW_RANDOM_INIT", "1")
    want = {"small": (512, 1024, 8, 6), "base": (768, 2048, 12, 12), "large": (1024, 2816, 24, 16)}
    for fam in ("google/t5-v1_1-", "google/flan-t5-"):
        for size, (d, ff, nl, nh) in want.items():
            cfg, sd = hf_io.resolve(fam + size, "t5")
            assert sd is None and (cfg.d_model, cfg.d_ff, cfg.num_layers, cfg.num_decoder_layers, cfg.num_heads, cfg.d_kv) == (d, ff, nl, nl, nh, 64)
            assert cfg.feed_forward_proj == "gated-gelu" and not cfg.tie_word_embeddings and not cfg.scale_decoder_outputs
    cfg, _ = hf_io.resolve("t5-small", "t5")
    assert cfg.feed_forward_proj == "relu" and cfg.tie_word_embeddings and cfg.scale_decoder_outputs
