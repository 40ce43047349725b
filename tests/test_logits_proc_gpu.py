"""Logits processors in MyModel.generate (repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_length, min_new_tokens) and
their kernel klab_logits_process_rows (csrc/logits_proc.hip): against the torch restatement of HF's processors
(tests/logits_proc_ref.py), against HF's own generate as the reference runs it (tests/golden/proc.npz from make_proc_goldens.py),
and the generate-level properties in all three loops."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

from tests.helpers import GOLD
from tests.logits_proc_ref import EOS, generate_processors, hf_process
from tests.sample_ref import boundary_tokens
from tests.test_sample_gpu import _build, _eos_row, _teacher_forced_logits, sample_rows

pytestmark = pytest.mark.gpu


def _lib():
    from klab_multimodalmodel_amd import _lib as L
    return L, L.load()


def process_rows(x, hist, row_div=1, log_softmax=False, pick=False, done=None, seq_out=None, repetition_penalty=1.0,
                 no_repeat_ngram_size=0, bad_words_ids=(), min_length=0, min_new_tokens=0, eos_id=EOS, pad_id=0):
    """klab_logits_process_rows over x ([R, V] fp32 / bf16, device) for rows = R * row_div with history hist [rows, cur_len]
    (position 0 = the start token); returns (processed [rows, V] f32, picked tokens [rows] or None) on the host"""
    L, lib = _lib()
    rows, cur = hist.shape
    V = x.shape[-1]
    seq = seq_out if seq_out is not None else torch.zeros(rows, cur + 1, dtype=torch.int64)
    seq[:, :cur] = hist
    seq_d = seq.cuda()
    out = torch.full((rows, V), float("nan"), device="cuda")
    tok = torch.full((rows,), -1, dtype=torch.int64, device="cuda")
    off = [0]
    for w in bad_words_ids:
        off.append(off[-1] + len(w))
    off_d = torch.tensor(off, dtype=torch.int32, device="cuda")
    tok_d = torch.tensor([t for w in bad_words_ids for t in w] or [0], dtype=torch.int32, device="cuda")
    stop = torch.zeros(1, dtype=torch.int32, device="cuda")
    done_d = done.cuda() if done is not None else None
    a = L.LogitsProcArgs()
    a.dtype, a.logits, a.ld, a.row_div, a.rows, a.V = L.dtype_code(x.dtype), x.data_ptr(), x.stride(0), row_div, rows, V
    a.log_softmax, a.seq, a.ld_seq, a.cur_len, a.start_id = int(log_softmax), seq_d.data_ptr(), seq.shape[1], cur, 0
    a.repetition_penalty, a.no_repeat_ngram_size, a.min_length, a.min_new_tokens, a.eos_id = (repetition_penalty, no_repeat_ngram_size,
                                                                                             min_length, min_new_tokens, eos_id)
    a.n_bad, a.bad_off, a.bad_tok = len(bad_words_ids), off_d.data_ptr(), tok_d.data_ptr()
    a.out, a.ld_out = out.data_ptr(), V
    if pick:
        a.pick, a.done, a.pad_id, a.tokens, a.stop_word = 1, done_d.data_ptr() if done_d is not None else None, pad_id, tok.data_ptr(), stop.data_ptr()
    L.check(lib.klab_logits_process_rows(C.byref(a), L.stream_ptr()), "klab_logits_process_rows")
    torch.cuda.synchronize()
    if seq_out is not None:
        seq_out.copy_(seq_d.cpu())
    if done is not None:
        done.copy_(done_d.cpu())
    return out.cpu(), (tok.cpu() if pick else None)


SETTINGS = [
    dict(repetition_penalty=1.3),
    dict(repetition_penalty=0.6, no_repeat_ngram_size=2),
    dict(no_repeat_ngram_size=1, min_length=9),
    dict(bad_words_ids=[[3], [2, 5], [4, 4, 4], [6] * 20]),
    dict(repetition_penalty=1.2, no_repeat_ngram_size=3, bad_words_ids=[[2, 3, 4], [0, 2]], min_length=4, min_new_tokens=6),
]


# ---- klab_logits_process_rows against the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("V", [384, 32128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("log_softmax", [False, True])
def test_process_rows_matches_restatement(V, dtype, log_softmax):
    g = torch.Generator().manual_seed(V + int(log_softmax))
    for row_div in (1, 3):
        R = 4
        x = (torch.randn(R, V, generator=g) * 3.0).to(dtype)
        for cur in (1, 2, 3, 7, 12):
            hist = torch.randint(0, 8, (R * row_div, cur), generator=g)
            hist[:, 0] = 0
            hist[1, 1:] = torch.tensor([2, 3] * cur)[:cur - 1]  # repeats
            for kw in SETTINGS:
                got, tok = process_rows(x.cuda(), hist, row_div=row_div, log_softmax=log_softmax, pick=True, **kw)
                want = hf_process(hist, x.float().repeat_interleave(row_div, 0), log_softmax=log_softmax, **kw)
                what = (V, dtype, log_softmax, row_div, cur, kw)
                assert torch.equal(torch.isinf(got), torch.isinf(want)), what
                fin = ~torch.isinf(want)
                if log_softmax:
                    assert torch.allclose(got[fin], want[fin], rtol=1e-6, atol=2e-6), what
                else:
                    assert torch.allclose(got[fin], want[fin], rtol=1e-6, atol=0), what
                assert torch.equal(tok, torch.argmax(got, -1)), what  # the pick is the arg-max of the processed row
                top2 = torch.topk(want, 2, -1)[0]
                clear = (top2[:, 0] - top2[:, 1]) > 1e-4
                assert torch.equal(tok[clear], torch.argmax(want, -1)[clear]), what


def test_process_rows_pick_bookkeeping():
    V = 64
    x = torch.full((4, V), -1.0)
    x[:, 9] = 2.0
    x[1, EOS] = 5.0       # row 1 picks EOS
    x[3] = -float("inf")  # banned everywhere below: picks 0
    hist = torch.zeros(4, 1, dtype=torch.int64)
    done = torch.tensor([0, 0, 1, 0], dtype=torch.int32)
    seq = torch.full((4, 3), -7, dtype=torch.int64)
    _, tok = process_rows(x.cuda(), hist, pick=True, done=done, seq_out=seq, pad_id=0)
    assert tok.tolist() == [9, EOS, 0, 0]
    assert done.tolist() == [0, 1, 1, 0]
    assert seq[:, 1].tolist() == [9, EOS, 0, 0] and (seq[:, 0] == 0).all()
    # min_length bans EOS: row 1 then picks 9
    _, tok = process_rows(x.cuda(), hist, pick=True, min_length=3)
    assert tok.tolist() == [9, 9, 9, 0]


def test_process_rows_rejects_oversized():
    with pytest.raises(NotImplementedError):
        process_rows(torch.zeros(1, 32769, device="cuda"), torch.zeros(1, 1, dtype=torch.int64))


# ---- generate against HF's generate --------------------------------------------------------------------------------------------
def _gold():
    return np.load(os.path.join(GOLD, "proc.npz")), json.load(open(os.path.join(GOLD, "proc.json")))


def _models():
    cache = {}

    def get(cs):
        key = (cs["model"], cs["variant"])
        if key not in cache:
            cache[key] = _build(cs["model"], "fp32", _eos_row(cs["model"]) if cs["variant"] == "eos" else None)
        return cache[key]
    return get


def test_generate_greedy_and_beam_match_reference():
    z, meta = _gold()
    cases = [c for c in meta["cases"] if c["mode"] != "sample"]
    assert len(cases) >= 60
    get = _models()
    for cs in cases:
        m, g = get(cs)
        pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
        want = torch.from_numpy(z[cs["id"] + ".seq"])
        if cs["mode"] == "greedy":
            got = m.generate(pix, src, max_length=cs["max_length"], **cs["kwargs"]).cpu()
            assert torch.equal(got, want), (cs["id"], got, want)
        else:
            got, sc = m.generate(pix, src, max_length=cs["max_length"], num_beams=cs["num_beams"], return_scores=True, **cs["kwargs"])
            assert torch.equal(got.cpu(), want), (cs["id"], got, want)
            ws = torch.from_numpy(z[cs["id"] + ".scores"])
            assert torch.allclose(sc.cpu(), ws, atol=1e-4, rtol=0), (cs["id"], sc, ws)


def _step_kept(logits, seq, t, kw, temperature, top_k):
    """the kept set of step t (the token at position t + 1) of the processors + warpers over teacher-forced logits"""
    hist = seq[:, :t + 1]
    proc, _ = process_rows(logits[:, t].contiguous().cuda(), hist, **kw)
    _, warped = sample_rows(proc.cuda(), temperature, top_k, 1.0, u=torch.zeros(proc.shape[0], device="cuda"))
    return proc, ~torch.isinf(warped)


def _engine_kw(kwargs):
    kw = generate_processors(kwargs)
    kw["bad_words_ids"] = [w for w in (kw.get("bad_words_ids") or []) if w != [EOS]]
    kw["min_new_tokens"] = kw.get("min_new_tokens") or 0
    return kw


def test_generate_sample_matches_reference_kept_sets():
    z, meta = _gold()
    cases = [c for c in meta["cases"] if c["mode"] == "sample"]
    assert len(cases) >= 40
    get = _models()
    boundary = own = 0
    for cs in cases:
        m, g = get(cs)
        pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
        seq = torch.from_numpy(z[cs["id"] + ".seq"])
        V, t_, k_ = cs["vocab"], cs.get("temperature", 1.0), cs["top_k"]
        want = np.unpackbits(z[cs["id"] + ".kept"], axis=-1)[..., :V].astype(bool)
        lg = _teacher_forced_logits(m, pix, src, seq, 1)
        kw = _engine_kw(cs["kwargs"])
        live = torch.from_numpy(np.cumsum(np.cumsum(seq[:, 1:].numpy() == EOS, 1), 1) <= 1)
        for t in range(seq.shape[1] - 1):
            proc, got = _step_kept(lg, seq, t, kw, t_, k_)
            diff = (got != torch.from_numpy(want[:, t])) & live[:, t:t + 1]
            if diff.any():
                ok = boundary_tokens(proc, t_, k_, 1.0)
                assert not (diff & ~ok).any(), (cs["id"], t, torch.nonzero(diff & ~ok)[:8])
                boundary += int(diff.any(-1).sum())
        # our own generate: every emitted token (through its row's EOS) lies in its step's kept set
        torch.manual_seed(own)
        own += 1
        ours = m.generate(pix, src, max_length=cs["max_length"], do_sample=True, temperature=t_, top_k=k_, **cs["kwargs"]).cpu()
        lg2 = _teacher_forced_logits(m, pix, src, ours, 1)
        live2 = np.cumsum(np.cumsum(ours[:, 1:].numpy() == EOS, 1), 1) <= 1
        for t in range(ours.shape[1] - 1):
            _, got = _step_kept(lg2, ours, t, kw, t_, k_)
            inside = got.gather(1, ours[:, t + 1:t + 2]).squeeze(1)
            assert inside[torch.from_numpy(live2[:, t])].all(), (cs["id"], t)
    assert boundary <= len(cases) // 10, boundary


# ---- properties at configs[1] shapes -----------------------------------------------------------------------------------------
def _configs1_model():
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
    return m, pix, src


def _check_rows(out, n, bad, min_len):
    for row in out.tolist():
        body = row[1:row.index(EOS, 1) + 1] if EOS in row[1:] else row[1:]
        toks = [0] + body
        if EOS in body:
            assert len(toks) - 1 >= min_len, row  # EOS at position p is chosen at cur_len p: p >= min_len
        grams = [tuple(toks[i:i + n]) for i in range(len(toks) - n + 1)]
        assert len(grams) == len(set(grams)), row
        for w in bad:
            for i in range(1, len(toks) - len(w) + 1):
                assert toks[i:i + len(w)] != w, (row, w)


def test_generate_properties_bf16_configs1_shapes():
    m, pix, src = _configs1_model()
    base = m.generate(pix, src, max_length=20).cpu()
    body = base[:, 1:].flatten().tolist()
    frequent = max(set(body), key=body.count)
    r0 = base[0, 1:].tolist()
    bad = [[frequent], [r0[3], r0[4]]]
    for loop in (dict(), dict(num_beams=4), dict(do_sample=True)):
        for kw, min_len in ((dict(no_repeat_ngram_size=3, bad_words_ids=bad, min_length=8), 8),
                            (dict(no_repeat_ngram_size=2, repetition_penalty=1.2, min_new_tokens=5, min_length=2), 6)):
            torch.manual_seed(0)
            out = m.generate(pix, src, max_length=20, **loop, **kw).cpu()
            assert out.shape[0] == 64 and 2 <= out.shape[1] <= 20 and (out[:, 0] == 0).all(), (loop, kw)
            assert ((out >= 0) & (out < m.main_cfg.vocab_size)).all()
            _check_rows(out, kw["no_repeat_ngram_size"], kw.get("bad_words_ids", []), min_len)
    # the processors bite: the plain greedy output of this random-init model repeats n-grams
    with pytest.raises(AssertionError):
        _check_rows(base, 3, [], 0)


def test_min_length_holds_back_eos():
    m, g = _build("tiny_b", "fp32", _eos_row("tiny_b"))
    pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
    plain = m.generate(pix, src, max_length=12).cpu()
    assert (plain[:, 1:] == EOS).any()
    for loop in (dict(), dict(num_beams=2), dict(do_sample=True, top_k=1)):
        for kw, first in ((dict(min_length=6), 6), (dict(min_new_tokens=7, min_length=3), 8)):
            out = m.generate(pix, src, max_length=12, **loop, **kw).cpu()
            for row in out.tolist():
                if EOS in row[1:]:
                    assert row.index(EOS, 1) >= first, (loop, kw, row)


# ---- the new path with neutral settings, isolation, errors ------------------------------------------------------------------
NEUTRAL = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=[], min_length=0, min_new_tokens=0)


def test_neutral_processors_match_plain_paths():
    for name in ("tiny_a", "tiny_b"):
        m, g = _build(name, "fp32", _eos_row(name))
        pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
        greedy = m.generate(pix, src, max_length=12, kv_cache=False)  # the host loop over the whole prefix: the independent path
        forced = m._generate_sample(pix, src, 12, 1, 1.0, 0, 1.0, dict(NEUTRAL), pick=True)
        assert torch.equal(greedy, forced), (name, greedy, forced)
        assert torch.equal(m.generate(pix, src, max_length=12), greedy), name
        a, sa = m.generate(pix, src, max_length=12, num_beams=4, return_scores=True)
        b, sb = m._generate_beam(pix, src, 12, 4, 1.0, False, 1, True, dict(NEUTRAL))
        assert torch.equal(a, b) and torch.allclose(sa, sb, atol=1e-5, rtol=0), (name, a, b)
        torch.manual_seed(3)
        c = m.generate(pix, src, max_length=12, do_sample=True, temperature=1.5, top_k=0)
        torch.manual_seed(3)
        d = m._generate_sample(pix, src, 12, 1, 1.5, 0, 1.0, dict(NEUTRAL))
        assert torch.equal(c, d), (name, c, d)


def test_processors_cleared_after_call_and_training_binding_kept():
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
    pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
    la, ga = step(m, g)
    lb, gb = step(m0, g)
    m.transformer.train()
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=[[5]], min_length=5)
    for loop in (dict(), dict(num_beams=3), dict(do_sample=True)):
        m.generate(pix, src, max_length=10, **loop, **kw)
        assert m.transformer.training
    # a plain call after them runs without processors
    for loop in (dict(num_beams=3), dict(do_sample=True, top_k=1)):
        torch.manual_seed(0)
        x = m.generate(pix, src, max_length=10, **loop)
        torch.manual_seed(0)
        y = m0.generate(pix, src, max_length=10, **loop)
        assert torch.equal(x, y), loop
    la2, ga2 = step(m, g)
    lb2, gb2 = step(m0, g)
    assert la == lb and la2 == lb2 and la2 == la
    assert torch.allclose(ga, gb, atol=1e-6, rtol=1e-5)
    assert torch.allclose(ga2, gb2, atol=1e-6, rtol=1e-5)


def test_generate_processor_argument_errors():
    m, g = _build("tiny_b", "fp32")
    pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
    with pytest.raises(ValueError, match="runs on the K/V cache only|run on the K/V cache only"):
        m.generate(pix, src, kv_cache=False, no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="strictly positive float"):
        m.generate(pix, src, repetition_penalty=0.0)
    with pytest.raises(ValueError, match="strictly positive integer"):
        m.generate(pix, src, num_beams=2, no_repeat_ngram_size=1.5)
    with pytest.raises(ValueError, match="The model vocabulary size is 512"):
        m.generate(pix, src, do_sample=True, bad_words_ids=[[3], [512]])
    with pytest.raises(NotImplementedError):
        m.generate(pix, src, bad_words_ids=[[a, b] for a in (2, 3) for b in range(300)])  # 1200 tokens
    # the processors' own K/V-cache message; beam and sampling keep theirs
    with pytest.raises(ValueError, match="kv_cache=True"):
        m.generate(pix, src, kv_cache=False, min_length=5)
    # kv_cache=False without processors still runs
    m.generate(pix, src, max_length=6, kv_cache=False, min_length=1)
