"""Forced decoding, the part that needs no GPU: the C struct mirror of klab_force_args, the argument errors of MyModel.score and of
generate(decoder_input_ids=...), the host-side min_new_tokens mapping for a decoder prompt, and the fixture recorded from the
reference (tests/golden/force.npz, make_force_goldens.py)."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

from tests.helpers import GOLD, load_golden

EOS = 1


def _model():
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_golden("tiny_b")
    sw = SwinConfig.from_dict(g["meta"]["swin_config"])
    t5 = T5Config.from_dict(g["meta"]["t5_config"])
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], g["sds"]["main"]), dtype="fp32")
    return m, g["inputs"]["pixel_values"], g["inputs"]["src_ids"]


def test_force_args_mirror_has_the_c_size():
    from klab_multimodalmodel_amd import _lib as L
    from klab_multimodalmodel_amd import engine
    lib = L.load()
    assert lib.klab_sizeof_force_args() == C.sizeof(L.ForceArgs)
    assert "klab_force_rows" in L.SIGNATURES and "klab_engine_gen_set_forced" in engine.ENGINE_SIGS
    assert engine.Engine.GEN_MODES["force"] == L.GEN_FORCE == 3
    cfg = engine.Engine.gen_cfg("force", 5, 7, 1, 0, want_logprobs=True)
    assert (cfg.mode, cfg.n, cfg.max_length, cfg.want_logprobs) == (3, 5, 7, 1)


def test_score_argument_errors():
    """every check runs before anything touches a device"""
    m, pix, src = _model()
    B, V = src.shape[0], m.main_cfg.vocab_size
    ok = torch.full((B, 3, 4), 5, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"\[B, N, L\]"):
        m.score(pix, src, ok[:, 0])  # rank 2
    with pytest.raises(ValueError, match=r"\[B, N, L\]"):
        m.score(pix, src, ok.int())
    with pytest.raises(ValueError, match="images"):
        m.score(pix, src, ok[:1].repeat(B + 1, 1, 1))
    with pytest.raises(ValueError, match="between 1 and 64"):
        m.score(pix, src, torch.full((B, 65, 4), 5, dtype=torch.int64))
    with pytest.raises(ValueError, match="between 1 and 64"):
        m.score(pix, src, torch.zeros((B, 0, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="at least one token"):
        m.score(pix, src, torch.zeros((B, 3, 0), dtype=torch.int64))
    for top in (0, 4, 1.0):
        with pytest.raises(ValueError, match="`top`"):
            m.score(pix, src, ok, top=top)
    for bad in (-1, V):
        c = ok.clone()
        c[0, 1, 2] = bad
        with pytest.raises(ValueError, match="outside"):
            m.score(pix, src, c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the arguments are fine: only now would the device be needed
        m.score(pix, src, ok, top=3)


def test_generate_decoder_prompt_argument_errors():
    """every check runs before anything touches a device"""
    m, pix, src = _model()
    B, V = src.shape[0], m.main_cfg.vocab_size
    p = torch.full((B, 3), 7, dtype=torch.int64)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(pix, src, num_beams=2, decoder_input_ids=p)
    with pytest.raises(ValueError, match="kv_cache"):
        m.generate(pix, src, kv_cache=False, decoder_input_ids=p)
    with pytest.raises(ValueError, match="return_logprobs"):
        m.generate(pix, src, return_logprobs=True, decoder_input_ids=p)
    with pytest.raises(ValueError, match="best_of"):
        m.generate(pix, src, do_sample=True, best_of=4, decoder_input_ids=p)
    with pytest.raises(ValueError, match=r"\[2, P\]"):
        m.generate(pix, src, decoder_input_ids=p[0])
    with pytest.raises(ValueError, match=r"\[2, P\]"):
        m.generate(pix, src, decoder_input_ids=p[:1])
    with pytest.raises(ValueError, match=r"\[2, P\]"):
        m.generate(pix, src, decoder_input_ids=p.int())
    for bad in (-1, V):
        q = p.clone()
        q[1, 1] = bad
        with pytest.raises(ValueError, match="outside"):
            m.generate(pix, src, decoder_input_ids=q)
    # HF's length check counts the start token it prepends: 3 + 1 >= 4
    with pytest.raises(ValueError, match="Input length of decoder_input_ids is 4, but `max_length` is set to 4"):
        m.generate(pix, src, max_length=4, decoder_input_ids=p)
    # ... and not one that is there already (column 0 is the start token in every row): 3 >= 3, but 3 < 4 is accepted as far as the device
    q = p.clone()
    q[:, 0] = m.main_cfg.decoder_start_token_id
    with pytest.raises(ValueError, match="Input length of decoder_input_ids is 3, but `max_length` is set to 3"):
        m.generate(pix, src, max_length=3, decoder_input_ids=q)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.generate(pix, src, max_length=4, decoder_input_ids=q)
    q[1, 0] = 7
    with pytest.raises(ValueError, match="some rows only"):
        m.generate(pix, src, decoder_input_ids=q)
    assert B == 2


@pytest.mark.parametrize("Lp", [1, 4])
def test_min_new_tokens_counts_from_the_prompt(Lp):
    """HF: min_new_tokens replaces min_length by min_new_tokens + prompt length; MinNewTokensLength bans EOS while
    cur_len - prompt length < min_new_tokens.  The kernel's test is cur_len - 1 < its own min_new_tokens."""
    from klab_multimodalmodel_amd.logits_proc import logits_processor_settings as S
    kw = dict(eos_token_id=EOS, vocab_size=100)
    got = S(1.0, 0, None, 0, 3, prompt_length=Lp, **kw)
    assert got["min_length"] == 3 + Lp and got["min_new_tokens"] == 3 + Lp - 1
    for cur_len in range(Lp, Lp + 6):  # the kernel's ban == HF's
        assert (cur_len - 1 < got["min_new_tokens"]) == (cur_len - Lp < 3)
    if Lp == 1:  # the default is today's mapping
        assert got == S(1.0, 0, None, 0, 3, **kw)
        assert S(1.0, 0, None, 5, None, **kw) == S(1.0, 0, None, 5, None, prompt_length=1, **kw)
    # without min_new_tokens the prompt changes nothing
    assert S(1.3, 2, None, 5, None, prompt_length=Lp, **kw) == S(1.3, 2, None, 5, None, **kw)
    assert S(1.0, 0, None, 0, None, prompt_length=Lp, **kw) is None


def test_force_goldens_are_consistent():
    z = np.load(os.path.join(GOLD, "force.npz"))
    meta = json.load(open(os.path.join(GOLD, "force.json")))
    N, L = meta["n"], meta["length"]
    assert (N, L) == (5, 6) and {mm["id"] for mm in meta["models"]} == {"tiny_b.plain", "tiny_b.eos", "tiny_v11_a.plain"}
    for mm in meta["models"]:
        cand, lp = z[mm["id"] + ".cand"], z[mm["id"] + ".cand_logprobs"]
        assert cand.shape == lp.shape == (mm["B"], N, L) and lp.dtype == np.float64 and (lp < 0).all()
        assert cand.min() >= 0 and cand.max() < mm["vocab"]
        first = [[(row == EOS).argmax() + 1 if (row == EOS).any() else L for row in img] for img in cand]
        assert all(f == [1, L, L, 3, 4] for f in first)
        assert not (cand[:, 2] == EOS).any() and (cand[:, 3, 3:] > 1).all() and (cand[:, 4, 4:] == 0).all()
        live = np.arange(L)[None, None] < np.asarray(first)[..., None]
        total = np.where(live, lp, 0.0).sum(-1)
        for penalty in (0, 1):
            sc = total / np.asarray(first, dtype=np.float64) ** penalty
            gaps = np.abs(sc[..., None] - sc[:, None]) + np.eye(N) * 1e9
            assert gaps.min() > meta["gap"]
            assert np.array_equal(z[mm["id"] + f".cand_order{penalty}"], np.argsort(-sc, -1))
    cases = meta["cases"]
    assert len(cases) == 18 and {c["prompt"] for c in cases} == {"p1", "p3"}
    goes_on = 0
    for cs in cases:
        prompt, seq = z[cs["id"] + ".prompt"], z[cs["id"] + ".seq"]
        P = prompt.shape[1]
        assert P == {"p1": 1, "p3": 3}[cs["prompt"]] and seq.shape[1] == cs["length"] <= meta["max_length"]
        assert (seq[:, 0] == 0).all() and np.array_equal(seq[:, 1:1 + P], prompt)
        if cs["prompt"] == "p3":
            assert (prompt == EOS).any(1).all()
            goes_on += int((seq[:, 1 + P:] > 1).any())
        if cs["kwargs"].get("min_new_tokens"):
            assert not (seq[:, 1 + P:1 + P + 3] == EOS).any()
    assert goes_on >= 1
