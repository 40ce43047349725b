"""Cross-attention maps, the part that needs no GPU: the argument errors of generate / score (return_cross_attention=True), the new
entry points (exported, listed, klab_gen_cfg untouched), the kernel's argument checks (they come before anything touches a
device), tests/xattn_ref.py against the fixture recorded from the reference (tests/golden/xattn.npz, make_xattn_goldens.py), and
the proofs tests/test_xattn_gpu.py takes for granted: the exact fixtures are exact (also through an f32 evaluation) and an f32
evaluation of random operands lies inside the per-element bound."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from klab_multimodalmodel_amd.ops import decode_attn_map  # noqa: F401  (the feature under test: without it this file proves nothing)
from tests import xattn_ref as X
from tests.helpers import GOLD, load_golden

EOS = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_argument_errors():
    """every check runs before anything touches a device"""
    m, pix, src = _model()
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(pix, src, num_beams=2, return_cross_attention=True)
    with pytest.raises(ValueError, match="kv_cache"):
        m.generate(pix, src, kv_cache=False, return_cross_attention=True)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(pix, src, num_beams=3, kv_cache=False, return_cross_attention=True)
    # the arguments are fine: only now would the device be needed
    for kw in (dict(), dict(return_logprobs=True), dict(do_sample=True, best_of=3), dict(repetition_penalty=1.3),
               dict(decoder_input_ids=torch.full((src.shape[0], 2), 7, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.generate(pix, src, return_cross_attention=True, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.score(pix, src, torch.full((src.shape[0], 3, 4), 5, dtype=torch.int64), return_cross_attention=True)
    with pytest.raises(ValueError, match=r"\[B, N, L\]"):
        m.score(pix, src, torch.full((src.shape[0], 4), 5, dtype=torch.int64), return_cross_attention=True)
    import inspect
    from klab_multimodalmodel_amd.models.model import MyModel
    for fn in (MyModel.generate, MyModel.score):  # the keyword is the last one and off by default
        p = list(inspect.signature(fn).parameters.values())[-1]
        assert p.name == "return_cross_attention" and p.default is False


def test_new_symbols_are_exported_and_listed():
    from klab_multimodalmodel_amd import _lib as L
    from klab_multimodalmodel_amd import engine
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "klab_mm.h")).read()
    assert len(L.SIGNATURES["klab_t5_decode_attn_map"]) == 18
    for name in ("klab_t5_decode_attn_map", "klab_engine_gen_attn_bytes", "klab_engine_gen_set_attn"):
        assert getattr(lib, name) is not None
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in L.SIGNATURES or name in engine.ENGINE_SIGS, name
    assert engine.ENGINE_SIGS["klab_engine_gen_attn_bytes"][1] is C.c_size_t
    assert callable(engine.Engine.gen_attn_bytes) and callable(engine.Engine.gen_set_attn)
    from klab_multimodalmodel_amd import ops
    assert callable(ops.decode_attn_map) and "klab_t5_decode_attn_map" in ops.decode_attn_map.__doc__


def test_gen_cfg_is_unchanged():
    """the maps are armed by a setter: klab_gen_cfg keeps its fields and its size"""
    from klab_multimodalmodel_amd import _lib as L
    lib = L.load()
    assert [f[0] for f in L.GenCfg._fields_] == ["mode", "n", "max_length", "eos_id", "pad_id", "temperature", "top_k", "top_p", "seed",
                                                 "length_penalty", "early_stopping", "procs", "want_logprobs"]
    assert lib.klab_sizeof_gen_cfg() == C.sizeof(L.GenCfg)
    assert hasattr(lib, "klab_engine_gen_set_attn")  # (what makes this test new: the setter is how they are armed)


def test_kernel_argument_errors_need_no_device():
    """bad arguments are refused before the launch: nothing here is a device address, and nothing is read"""
    from klab_multimodalmodel_amd import _lib as L
    lib = L.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def call(dtype=L.F32, q=p, q_bstride=16, q_div=1, k=p, kv_bstride=64, ldk=16, kv_group=1, bias=None, bias_ld=0, done=None, out=p,
             out_bstride=4, R=2, H=2, Lk=4, dk=8):
        return lib.klab_t5_decode_attn_map(dtype, q, q_bstride, q_div, k, kv_bstride, ldk, kv_group, bias, bias_ld, done, out, out_bstride,
                                           R, H, Lk, dk, None)
    for kw in (dict(q=None), dict(k=None), dict(out=None), dict(R=0), dict(R=-1), dict(H=0), dict(Lk=0), dict(q_div=0), dict(kv_group=0),
               dict(out_bstride=3), dict(bias=p, bias_ld=3), dict(dtype=2), dict(dtype=-1)):
        assert call(**kw) == L.ERR_BADARG, kw
    for dk in (0, 4, 12, 24, 48, 96, 256):
        assert call(dk=dk) == L.ERR_UNSUPPORTED, dk
        assert call(dk=dk, dtype=L.BF16) == L.ERR_UNSUPPORTED, dk


# ---- the fixture and its restatement -------------------------------------------------------------------------------------------------
def _gold():
    return np.load(os.path.join(GOLD, "xattn.npz")), json.load(open(os.path.join(GOLD, "xattn.json")))


def test_xattn_goldens_are_consistent():
    z, meta = _gold()
    force = np.load(os.path.join(GOLD, "force.npz"))
    assert {mm["id"] for mm in meta["models"]} == {"tiny_b.plain", "tiny_b.eos", "tiny_v11_a.plain"}
    assert os.path.getsize(os.path.join(GOLD, "xattn.npz")) < 1 << 20
    for mm in meta["models"]:
        mid = mm["id"]
        cand, maps, ids, gm = force[mid + ".cand"], z[mid + ".cand_maps"], z[mid + ".greedy_ids"], z[mid + ".greedy_maps"]
        B, N, L = cand.shape
        assert maps.dtype == gm.dtype == np.float64 and maps.shape == (B, N, mm["n_dec_layers"], L, mm["Le"])
        assert gm.shape == (B, mm["n_dec_layers"], ids.shape[1] - 1, mm["Le"]) and 2 <= ids.shape[1] <= meta["max_length"]
        assert (ids[:, 0] == 0).all() and ids.shape[1] == mm["greedy_length"]
        for a in (maps, gm):  # probabilities: every position of every layer sums to 1
            assert (a >= 0).all() and np.abs(a.sum(-1) - 1).max() < 1e-12
        assert 0 < mm["d32"] < 2.0 ** -20 and 0 < mm["image_tokens"] < mm["Le"]
        assert z[mm["model"] + ".enc_out"].shape[:2] == (B, mm["Le"])
        # the maps look at the image: the image tokens do not all get the same weight
        assert maps[..., :mm["image_tokens"]].std(-1).min() > 0


@pytest.mark.parametrize("mid", ["tiny_b.plain", "tiny_b.eos", "tiny_v11_a.plain"])
def test_reference_restatement_reproduces_the_goldens(mid):
    """tests/xattn_ref.py on the stored weights and the stored encoder output against HF's own cross_attentions (float64, eager)"""
    z, meta = _gold()
    sd, cfg = X.golden_weights(mid)
    enc = torch.from_numpy(z[mid.rsplit(".", 1)[0] + ".enc_out"])
    cand = torch.from_numpy(np.load(os.path.join(GOLD, "force.npz"))[mid + ".cand"])
    B, N, L = cand.shape
    got = X.decoder_cross_attention(sd, cfg, enc.repeat_interleave(N, 0), cand.view(B * N, L))
    err = float((got.view(B, N, *got.shape[1:]) - torch.from_numpy(z[mid + ".cand_maps"])).abs().max())
    ids = torch.from_numpy(z[mid + ".greedy_ids"])
    gerr = float((X.decoder_cross_attention(sd, cfg, enc, ids[:, 1:]) - torch.from_numpy(z[mid + ".greedy_maps"])).abs().max())
    print(f"{mid}: restatement vs HF float64, candidates {err:.3e}, greedy {gerr:.3e}")
    assert err <= 1e-10 and gerr <= 1e-10, (err, gerr)
    # ... and evaluated in fp32 it is as far from them as the reference's own fp32 run is (the same order of magnitude)
    d32 = next(mm["d32"] for mm in meta["models"] if mm["id"] == mid)
    f32 = X.decoder_cross_attention(sd, cfg, enc.float().repeat_interleave(N, 0), cand.view(B * N, L), dtype=torch.float32)
    e32 = float((f32.double().view(B, N, *got.shape[1:]) - torch.from_numpy(z[mid + ".cand_maps"])).abs().max())
    print(f"{mid}: fp32 restatement {e32:.3e}, d32 {d32:.3e}")
    assert e32 <= 4 * d32 + 2.0 ** -20


def test_live_labels():
    c = torch.tensor([[5, 1, 7, 1], [1, 0, 0, 0], [4, 5, 6, 7]])
    assert X.live_labels(c, EOS).tolist() == [[True, True, False, False], [True, False, False, False], [True] * 4]


# ---- what the GPU test takes for granted -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", X.EXACT_KINDS)
def test_exact_fixtures_are_exact(kind, n):
    """the written-down map is what softmax gives in float64 AND in float32, bit for bit, it is a dyadic number float32 holds, the
    operands are bf16 values, and the heads of a row do choose different keys"""
    cases = X.exact_cases(kind)
    assert {c[0] for c in cases} == set(X.EXACT_H) and {c[1] for c in cases} == set(X.EXACT_DK) and {c[3] for c in cases} == set(X.GROUPS)
    assert {c[2] for c in cases} == set(X.EXACT_LK)
    spread = 0
    for H, dk, Lk, groups in cases:
        for pos in range(3):
            q_src, k_src, bias, want = X.exact_operands(kind, n, H, dk, Lk, groups, pos)
            what = (kind, H, dk, Lk, groups, pos)
            for t in (q_src, k_src) + (() if bias is None else (bias,)):
                assert torch.equal(t.to(torch.bfloat16).double(), t), what
            q, k = X.per_row(q_src, k_src, groups)
            assert q.shape == (X.R, H, dk) and k.shape == (X.R, H, Lk, dk)
            m64, P = X.head_mean_map(q, k, bias)
            assert float((m64 - want).abs().max()) <= 1e-40, what  # (exp(-128) is not 0 in float64; nothing else is off)
            m32, _ = X.head_mean_map(q.float(), k.float(), None if bias is None else bias.float())
            assert m32.dtype == torch.float32 and torch.equal(m32.double(), want), what
            assert torch.equal(want.float().double(), want) and torch.equal(want * (4 * H), (want * (4 * H)).round()), what
            assert float((want.sum(-1) - 1).abs().max()) == 0.0, what
            spread += int(H > 1 and Lk > 4 and (P[0] > 0).any(0).sum() > (P[0, 0] > 0).sum())
    assert spread >= len(cases) // 2


def test_random_operands_in_f32_lie_inside_the_bound():
    assert {c[0] for c in X.RANDOM_CASES} == {6, 12, 32} and {c[3] for c in X.RANDOM_CASES} == set(X.GROUPS)
    for i, (H, dk, Lk, groups, with_bias) in enumerate(X.RANDOM_CASES):
        q_src, k_src, bias = X.random_operands(H, dk, Lk, groups, with_bias, i)
        q, k = X.per_row(q_src, k_src, groups)
        ref, P = X.head_mean_map(q, k, bias)
        bound = X.map_bound(q, k, P, Lk, dk)
        got, _ = X.head_mean_map(q.float(), k.float(), None if bias is None else bias.float())
        err = (got.double() - ref).abs()
        ratio = float((err / bound).max())
        print(f"H {H} dk {dk} Lk {Lk} {groups} bias {with_bias}: max err / bound {ratio:.3f}")
        assert (err <= bound).all(), (H, dk, Lk, ratio)
        assert float((got.double().sum(-1) - 1).abs().max()) <= X.row_sum_bound(Lk, H) and (got >= 0).all()
