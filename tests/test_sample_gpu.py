"""Sampling generation (MyModel.generate(do_sample=True)) and its kernel klab_sample_rows (csrc/sample.hip): against the torch
restatement of HF's warpers (tests/sample_ref.py), against HF's own `_sample` as the reference runs it (tests/golden/sample.npz
from make_sample_goldens.py), its draw distribution, and the generate-level properties."""
import ctypes as C
import itertools
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from tests.helpers import GOLD, load_golden
from tests.sample_ref import boundary_tokens, hf_warp, inverse_cdf

pytestmark = pytest.mark.gpu

TEMPERATURE = (0.7, 1.0, 1.5)
TOP_K = (0, 1, 5, 50)
TOP_P = (1.0, 0.9, 0.5)


def _lib():
    from klab_multimodalmodel_amd import _lib as L
    return L, L.load()


def _build(name, dtype, eos_row=None):
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_golden(name)
    sw = SwinConfig.from_dict(g["meta"]["swin_config"])
    t5 = T5Config.from_dict(g["meta"]["t5_config"])
    main = dict(g["sds"]["main"])
    if eos_row is not None:
        main["shared.weight"] = main["shared.weight"].clone()
        main["shared.weight"][1] = torch.from_numpy(eos_row)
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], main), dtype=dtype)
    return m.to("cuda"), g


def _eos_row(name):
    return np.load(os.path.join(GOLD, "beam.npz"))[f"{name}.eos_row"]


def sample_rows(x, temperature, top_k, top_p, u=None, row_div=1, rows=None, seed=0, step=1, ld=None, V=None, want_warped=True):
    """klab_sample_rows over x ([*, V] fp32 / bf16, device); returns (tokens [rows] int64, warped [rows, V] f32 or None)"""
    L, lib = _lib()
    V = V or x.shape[-1]
    rows = rows or x.shape[0]
    tok = torch.empty(rows, dtype=torch.int64, device="cuda")
    warped = torch.empty(rows, V, dtype=torch.float32, device="cuda") if want_warped else None
    a = L.SampleArgs()
    a.dtype, a.logits, a.ld, a.row_div, a.rows, a.V = L.dtype_code(x.dtype), x.data_ptr(), ld or x.stride(0), row_div, rows, V
    a.temperature, a.top_k, a.top_p, a.seed, a.step = temperature, top_k, top_p, seed, step
    a.u_in = u.data_ptr() if u is not None else None
    a.warped, a.ld_warped, a.tokens = warped.data_ptr() if want_warped else None, V, tok.data_ptr()
    L.check(lib.klab_sample_rows(C.byref(a), L.stream_ptr()), "klab_sample_rows")
    torch.cuda.synchronize()
    return tok.cpu(), warped.cpu() if want_warped else None


def _check_kept(warped, logits, t, k, p, what, limit):
    """the kernel's kept set equals the restatement's except for boundary tokens; returns the number of such differences"""
    ref = hf_warp(logits, t, k, p)
    kk, rk = ~torch.isinf(warped), ~torch.isinf(ref)
    diff = kk != rk
    if diff.any():
        ok = boundary_tokens(logits, t, k, p)
        assert not (diff & ~ok).any(), (what, torch.nonzero(diff & ~ok)[:8])
    both = kk & rk
    assert torch.allclose(warped[both], ref[both], rtol=1e-6, atol=0), what
    n = int(diff.any(-1).sum())
    assert n <= limit, (what, n)
    return n


# ---- klab_sample_rows against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [384, 32128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sample_rows_matches_restatement(V, dtype):
    g = torch.Generator().manual_seed(V)
    rows = 8
    x = torch.randn(rows, V, generator=g) * 3.0
    x[1] = (x[1] * 0.7).round()                 # a row full of exact ties
    x[2, torch.randperm(V, generator=g)[:3]] = 14.0  # a row dominated by a three-way tie at the max
    x[3] = x[3] * 0.05                          # a nearly flat row
    x = x.to(dtype)
    xd = x.cuda()
    boundary = near_step = 0
    for t, k, p in itertools.product(TEMPERATURE, TOP_K, TOP_P):
        u = torch.rand(rows, generator=g)
        tok, warped = sample_rows(xd, t, k, p, u=u.cuda())
        what = (V, dtype, t, k, p)
        boundary += _check_kept(warped, x.float(), t, k, p, what, rows)
        want, dist = inverse_cdf(warped, u)
        bad = tok != want
        assert not (bad & (dist > 1e-5)).any(), (what, tok, want, dist)
        near_step += int(bad.sum())
        assert (~torch.isinf(warped.gather(1, tok.view(-1, 1)))).all(), what  # never a removed token
    # the boundary allowances are exceptions, not the rule (row 1 is all ties, and bf16 logits tie often: HF's sort then splits the
    # tie group the top-p boundary falls in)
    combos = len(TEMPERATURE) * len(TOP_K) * len(TOP_P)
    assert boundary <= combos * (2 if dtype == torch.float32 else 4) and near_step <= 4, (boundary, near_step)


def test_sample_rows_rejects_oversized_vocabulary():
    L, lib = _lib()
    x = torch.zeros(1, 32769, device="cuda")
    with pytest.raises(NotImplementedError):
        sample_rows(x, 1.0, 0, 1.0)


# ---- the draw distribution ---------------------------------------------------------------------------------------------------
def _chi2_bound(df, z=4.0):
    """Wilson-Hilferty upper quantile of chi-square(df) at a normal deviate z (z = 4: about 3e-5)"""
    return df * (1.0 - 2.0 / (9 * df) + z * math.sqrt(2.0 / (9 * df))) ** 3


@pytest.mark.parametrize("t,k,p", [(1.0, 0, 1.0), (0.7, 50, 0.9), (1.5, 0, 0.5), (1.0, 5, 1.0)])
def test_sample_rows_distribution(t, k, p):
    g = torch.Generator().manual_seed(17)
    V, R = 1000, 1 << 16
    x = (torch.randn(1, V, generator=g) * 2.0).cuda()
    tok, _ = sample_rows(x, t, k, p, row_div=R, rows=R, seed=0x1234567890ABCDEF, step=3, want_warped=False)
    _, warped = sample_rows(x, t, k, p, rows=1)
    w = warped[0]
    kept = ~torch.isinf(w)
    counts = torch.bincount(tok, minlength=V).double()
    assert counts[~kept].sum() == 0  # no removed token is ever drawn
    prob = torch.softmax(w.double(), -1)
    exp = prob * R
    big = exp >= 5
    obs = torch.cat([counts[big], counts[~big & kept].sum().view(1)])
    ex = torch.cat([exp[big], exp[~big & kept].sum().view(1)])
    if ex[-1] < 5:
        obs, ex = obs[:-1], ex[:-1]
        obs[-1] += counts[~big & kept].sum()
        ex[-1] += exp[~big & kept].sum()
    chi2 = float(((obs - ex) ** 2 / ex).sum())
    df = len(ex) - 1
    assert df >= 1 or int(kept.sum()) == 1
    if df >= 1:
        assert chi2 < _chi2_bound(df), (chi2, df)


# ---- generate(do_sample=True) against HF's `_sample` ---------------------------------------------------------------------------
def _teacher_forced_logits(m, pix, src, seq, n):
    """fp32 logits [rows, L-1, V] of an evaluation-mode forward of the sequences (row b*n + j reads image b)"""
    tgt = seq[:, 1:].contiguous().cuda()
    pr, sr = pix.repeat_interleave(n, 0).contiguous(), src.repeat_interleave(n, 0).contiguous()
    eng = m._engine_for(pr, sr, tgt)
    eng.forward(pr, sr, tgt, training=0, seed=0, want_grad=False)
    return eng.buffer("logits").view(tgt.shape[0], tgt.shape[1], -1).clone()


def _upto_eos(tok, eos=1):
    return np.cumsum(np.cumsum(tok == eos, 1), 1) <= 1


def test_generate_sample_matches_reference_kept_sets():
    z = np.load(os.path.join(GOLD, "sample.npz"))
    cases = json.load(open(os.path.join(GOLD, "sample.json")))["cases"]
    assert len(cases) >= 400
    models = {}
    boundary = own = 0
    for cs in cases:
        key = (cs["model"], cs["variant"])
        if key not in models:
            models[key] = _build(cs["model"], "fp32", _eos_row(cs["model"]) if cs["variant"] == "eos" else None)
        m, g = models[key]
        pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
        t, k, p, n = cs["temperature"], cs["top_k"], cs["top_p"], cs["num_return_sequences"]
        rows, Lc, V = cs["rows"], cs["length"], cs["vocab"]
        seq = torch.from_numpy(z["seq"][cs["row0"]:cs["row0"] + rows, :Lc])
        want = np.unpackbits(z["kept"][cs["row0"]:cs["row0"] + rows, :Lc - 1], axis=-1)[..., :V].astype(bool)
        logits = _teacher_forced_logits(m, pix, src, seq, n).reshape(rows * (Lc - 1), V)
        _, warped = sample_rows(logits, t, k, p, u=torch.zeros(rows * (Lc - 1), device="cuda"))
        got = ~torch.isinf(warped)
        diff = got != torch.from_numpy(want.reshape(rows * (Lc - 1), V))
        if diff.any():
            ok = boundary_tokens(logits.cpu(), t, k, p)
            assert not (diff & ~ok).any(), (cs["id"], torch.nonzero(diff & ~ok)[:8])
            boundary += int(diff.any(-1).sum())
        # our own generate: every emitted token (through the row's EOS) lies in the kept set of its teacher-forced logits
        if n == 3 and t == 0.7:
            torch.manual_seed(len(cases) + own)
            ours = m.generate(pix, src, max_length=cs["max_length"], do_sample=True, temperature=t, top_k=k, top_p=p,
                              num_return_sequences=n).cpu()
            own += 1
            assert ours.shape[0] == rows and (ours[:, 0] == 0).all()
            lg = _teacher_forced_logits(m, pix, src, ours, n)
            steps = ours.shape[1] - 1
            _, w2 = sample_rows(lg.reshape(rows * steps, V), t, k, p, u=torch.zeros(rows * steps, device="cuda"))
            tok = ours[:, 1:]
            inside = ~torch.isinf(w2.view(rows, steps, V).gather(-1, tok.unsqueeze(-1)).squeeze(-1))
            assert inside[torch.from_numpy(_upto_eos(tok.numpy()))].all(), cs["id"]
    assert own >= 48
    assert boundary <= len(cases) // 20, boundary


# ---- properties ---------------------------------------------------------------------------------------------------------------
def test_generate_sample_top_k_1_is_greedy():
    m, g = _build("tiny_b", "fp32")
    pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
    a = m.generate(pix, src, max_length=12)
    b = m.generate(pix, src, max_length=12, do_sample=True, top_k=1)
    assert torch.equal(a, b), (a, b)
    lg = _teacher_forced_logits(m, pix, src, a.cpu(), 1)
    top2 = torch.topk(lg, 2, -1)[0]
    live = torch.from_numpy(_upto_eos(a[:, 1:].cpu().numpy()))
    assert (top2[..., 0] > top2[..., 1]).cpu()[live].all()  # no tie at the max: the pick is the arg-max on both paths


def test_generate_sample_seeding():
    m, g = _build("tiny_b", "fp32")
    pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
    kw = dict(max_length=12, do_sample=True, temperature=1.5, top_k=0, num_return_sequences=2)
    torch.manual_seed(5)
    a = m.generate(pix, src, **kw)
    c = m.generate(pix, src, **kw)
    torch.manual_seed(5)
    b = m.generate(pix, src, **kw)
    assert torch.equal(a, b)
    assert a.shape != c.shape or not torch.equal(a, c)


def test_generate_sample_num_return_sequences():
    m, g = _build("tiny_a", "fp32")
    pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
    B = src.shape[0]
    torch.manual_seed(0)
    out = m.generate(pix, src, max_length=10, do_sample=True, temperature=1.5, top_k=0, num_return_sequences=3)
    assert out.shape[0] == 3 * B and out.shape[1] <= 10
    assert (out[:, 0] == m.main_cfg.decoder_start_token_id).all()
    assert all(len({tuple(r) for r in out[b * 3:(b + 1) * 3].tolist()}) > 1 for b in range(B))
    assert ((out >= 0) & (out < m.main_cfg.vocab_size)).all()


def test_generate_sample_pads_after_eos_and_crops():
    ml = 20
    cropped = finished = 0
    for name in ("tiny_a", "tiny_b", "tiny_c"):
        m, g = _build(name, "fp32", _eos_row(name))
        pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
        cfg = m.main_cfg
        for s, (t, k) in enumerate(itertools.product((0.3, 0.7), (1, 5))):
            torch.manual_seed(s)
            out = m.generate(pix, src, max_length=ml, do_sample=True, temperature=t, top_k=k).cpu()
            for row in out.tolist():
                if cfg.eos_token_id in row[1:]:
                    finished += 1
                    e = row.index(cfg.eos_token_id, 1)
                    assert all(x == cfg.pad_token_id for x in row[e + 1:]), row
            if out.shape[1] < ml:
                cropped += 1
                # cropped right where the last row finished
                firsts = [row.index(cfg.eos_token_id, 1) for row in out.tolist()]
                assert max(firsts) == out.shape[1] - 1, out
    assert finished >= 1 and cropped >= 1, (finished, cropped)


def test_generate_sample_bf16_configs1_shapes():
    import bench
    from klab_multimodalmodel_amd.models.model import MyModel
    sw, t5 = bench.cfg2_configs()
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _seed=0, dtype="bf16").to("cuda")
    gen = torch.Generator().manual_seed(0)
    B = 64
    pix = torch.randn(B, 3, sw.image_size, sw.image_size, generator=gen).cuda()
    src = torch.randint(2, t5.vocab_size, (B, 16), generator=gen).cuda()
    for n in (1, 5):
        out = m.generate(pix, src, max_length=20, do_sample=True, num_return_sequences=n)
        assert out.shape[0] == B * n and 2 <= out.shape[1] <= 20
        assert ((out >= 0) & (out < t5.vocab_size)).all()


# ---- isolation and errors -----------------------------------------------------------------------------------------------------
def test_generate_sample_keeps_training_binding():
    """a sampling generate between two forward + backward steps changes neither their loss nor their gradients and restores
    transformer.training"""
    def step(m, g):
        inp = g["inputs"]
        m.transformer.eval()
        for p in m.transformer.parameters():
            p.grad = None
        loss = m({"pixel_values": inp["pixel_values"].cuda()}, {"input_ids": inp["src_ids"].cuda()}, {"input_ids": inp["tgt_ids"].cuda()})
        loss.backward()
        torch.cuda.synchronize()
        return float(loss), m.flat_grads().clone()

    m, g = _build("tiny_b", "fp32")
    m0, _ = _build("tiny_b", "fp32")
    la, ga = step(m, g)
    lb, gb = step(m0, g)
    inp = g["inputs"]
    m.transformer.train()
    m.generate(inp["pixel_values"].cuda(), inp["src_ids"].cuda(), max_length=10, do_sample=True, num_return_sequences=3)
    assert m.transformer.training
    la2, ga2 = step(m, g)
    lb2, gb2 = step(m0, g)
    assert la == lb and la2 == lb2 and la2 == la
    assert torch.allclose(ga, gb, atol=1e-6, rtol=1e-5)
    assert torch.allclose(ga2, gb2, atol=1e-6, rtol=1e-5)


def test_generate_sample_argument_errors():
    m, g = _build("tiny_b", "fp32")
    pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
    with pytest.raises(NotImplementedError, match="beam sampling"):
        m.generate(pix, src, do_sample=True, num_beams=2)
    with pytest.raises(ValueError, match="kv_cache"):
        m.generate(pix, src, do_sample=True, kv_cache=False)
    with pytest.raises(ValueError, match="return_scores"):
        m.generate(pix, src, do_sample=True, return_scores=True)
    for t in (0.0, -1.0):
        with pytest.raises(ValueError, match="has to be a strictly positive float"):
            m.generate(pix, src, do_sample=True, temperature=t)
    with pytest.raises(ValueError, match="top_k"):
        m.generate(pix, src, do_sample=True, top_k=-1)
    for p in (-0.1, 1.5):
        with pytest.raises(ValueError, match="top_p"):
            m.generate(pix, src, do_sample=True, top_p=p)
    # do_sample=False keeps every existing message
    with pytest.raises(ValueError, match=r"`num_return_sequences` \(3\) has to be smaller or equal to `num_beams` \(1\)"):
        m.generate(pix, src, num_return_sequences=3)
    m.transformer.eval()
    m.generate(pix, src, max_length=8, do_sample=True)
    assert not m.transformer.training
