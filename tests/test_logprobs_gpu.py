"""Per-token log-probabilities of greedy and sampled decoding (generate(return_logprobs=True), best_of): the two choosing kernels
with their `logprob` output (klab_sample_rows, klab_logits_process_rows with pick), klab_gen_finalize, the decoding session and
generate, against the float64 restatement (tests/logprob_ref.py) and against HF's compute_transition_scores as the reference
runs it (tests/golden/logprobs.npz from make_logprobs_goldens.py)."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

from tests.helpers import GOLD, load_golden
from tests.logits_proc_ref import hf_process
from tests.logprob_ref import sequence_scores, token_logprob, warped_scores

pytestmark = pytest.mark.gpu

EOS = 1
SAMPLE_SETTINGS = [(1.0, 0, 1.0), (0.7, 0, 1.0), (1.0, 3, 1.0), (1.0, 0, 0.6), (0.7, 3, 0.6)]  # temperature, top_k, top_p
PROC_SETTINGS = [
    dict(),
    dict(repetition_penalty=1.3),
    dict(no_repeat_ngram_size=2),
    dict(bad_words_ids=[[3], [2, 4]]),
    dict(min_length=9),
    dict(min_new_tokens=7),
    dict(repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=[[3], [2, 4]], min_length=9, min_new_tokens=7),
]
SENTINEL = 123.25  # fills the log-probability buffers: only the one column of the call may change


def _lib():
    from klab_multimodalmodel_amd import _lib as L
    return L, L.load()


def uniform_logits(rows, V, dtype, seed):
    """logits uniform in [-12, 12), rounded to dtype (the kernels and the restatement read the same rounded values)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(rows, V, generator=g) * 24.0 - 12.0).to(dtype)


def sample_inputs(V, dtype):
    """3 rows: a live row, a row finished on entry, and a row that draws EOS (token 0 the smallest score, EOS the largest, and a u
    just above 0: the running probability first exceeds it at EOS)"""
    x = uniform_logits(3, V, dtype, 1000 + V)
    x[2, 0], x[2, EOS] = -12.0, 12.0
    u = torch.tensor([0.37, 0.5, 1e-4])
    done = torch.tensor([0, 1, 0], dtype=torch.int32)
    return x, u, done


# ---- 1. klab_sample_rows ---------------------------------------------------------------------------------------------------
def sample_rows(x, u, done, t, k, p, pos, ld_seq, want_logprob, ld_logprob=None):
    L, lib = _lib()
    rows, V = x.shape
    xd, ud, dd = x.cuda(), u.cuda(), done.cuda()
    tok = torch.full((rows,), -1, dtype=torch.int64, device="cuda")
    warped = torch.empty(rows, V, dtype=torch.float32, device="cuda")
    seq = torch.full((rows, ld_seq), -7, dtype=torch.int64, device="cuda")
    stop = torch.zeros(1, dtype=torch.int32, device="cuda")
    ld_logprob = ld_logprob or ld_seq
    lp = torch.full((rows, ld_logprob), SENTINEL, dtype=torch.float32, device="cuda")
    a = L.SampleArgs()
    a.dtype, a.logits, a.ld, a.row_div, a.rows, a.V = L.dtype_code(x.dtype), xd.data_ptr(), xd.stride(0), 1, rows, V
    a.temperature, a.top_k, a.top_p, a.seed, a.step = t, k, p, 0, pos
    a.u_in, a.warped, a.ld_warped = ud.data_ptr(), warped.data_ptr(), V
    a.done, a.eos_id, a.pad_id, a.start_id = dd.data_ptr(), EOS, 0, 0
    a.tokens, a.seq, a.ld_seq, a.pos, a.stop_word = tok.data_ptr(), seq.data_ptr(), ld_seq, pos, stop.data_ptr()
    if want_logprob:
        a.logprob, a.ld_logprob = lp.data_ptr(), ld_logprob
    L.check(lib.klab_sample_rows(C.byref(a), L.stream_ptr()), "klab_sample_rows")
    torch.cuda.synchronize()
    return dict(tok=tok.cpu(), warped=warped.cpu(), done=dd.cpu(), seq=seq.cpu(), stop=stop.cpu(), logprob=lp.cpu())


def _same_old_outputs(a, b, what):
    for key in ("tok", "done", "seq", "stop"):
        assert torch.equal(a[key], b[key]), (what, key)
    for key in ("warped", "out"):
        if key in a:
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (what, key)


@pytest.mark.parametrize("V", [5, 1000, 32100, 32768])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sample_rows_logprob(V, dtype):
    x, u, done = sample_inputs(V, dtype)
    pos, ld = 3, 6
    for t, k, p in SAMPLE_SETTINGS:
        what = (V, dtype, t, k, p)
        ref, margin = warped_scores(x, t, k, p)
        assert margin > 1e-5, (what, margin)  # the inputs sit clear of the top-p boundary
        plain = sample_rows(x, u, done, t, k, p, pos, ld, False)
        got = sample_rows(x, u, done, t, k, p, pos, ld, True)
        _same_old_outputs(plain, got, what)
        assert (plain["logprob"] == SENTINEL).all(), what
        tok = got["tok"]
        assert tok.tolist()[1:] == [0, EOS] and got["done"].tolist() == [int(tok[0] == EOS), 1, 1], (what, tok)
        assert torch.equal(torch.isinf(got["warped"]), torch.isinf(ref)), what  # the restatement keeps what the kernel keeps
        want = token_logprob(ref, torch.tensor([int(tok[0]), 0, EOS]))
        lp = got["logprob"]
        assert float(lp[1, pos]) == 0.0, what  # finished on entry: the forced pad scores 0
        for r in (0, 2):
            assert torch.isfinite(want[r]) and abs(float(lp[r, pos]) - float(want[r])) <= 1e-5, (what, r, float(lp[r, pos]), float(want[r]))
        lp[:, pos] = SENTINEL
        assert (lp == SENTINEL).all(), what  # nothing but column pos is written


def test_sample_rows_logprob_needs_room():
    x, u, done = sample_inputs(5, torch.float32)
    with pytest.raises(ValueError):
        sample_rows(x, u, done, 1.0, 0, 1.0, 3, 6, True, ld_logprob=3)


# ---- 2. klab_logits_process_rows with pick -------------------------------------------------------------------------------------
def process_pick(x, hist, done, want_logprob, ld_logprob=None, **kw):
    L, lib = _lib()
    rows, cur = hist.shape
    V = x.shape[-1]
    bad = kw.get("bad_words_ids", ())
    seq = torch.full((rows, cur + 2), -7, dtype=torch.int64)
    seq[:, :cur] = hist
    xd, seq_d, dd = x.cuda(), seq.cuda(), done.cuda()
    out = torch.full((rows, V), float("nan"), device="cuda")
    tok = torch.full((rows,), -1, dtype=torch.int64, device="cuda")
    off = [0]
    for w in bad:
        off.append(off[-1] + len(w))
    off_d = torch.tensor(off, dtype=torch.int32, device="cuda")
    tok_d = torch.tensor([t for w in bad for t in w] or [0], dtype=torch.int32, device="cuda")
    stop = torch.zeros(1, dtype=torch.int32, device="cuda")
    ld_logprob = ld_logprob or cur + 2
    lp = torch.full((rows, ld_logprob), SENTINEL, dtype=torch.float32, device="cuda")
    a = L.LogitsProcArgs()
    a.dtype, a.logits, a.ld, a.row_div, a.rows, a.V = L.dtype_code(x.dtype), xd.data_ptr(), xd.stride(0), 1, rows, V
    a.log_softmax, a.seq, a.ld_seq, a.cur_len, a.start_id = 0, seq_d.data_ptr(), seq.shape[1], cur, 0
    a.repetition_penalty, a.no_repeat_ngram_size = kw.get("repetition_penalty", 1.0), kw.get("no_repeat_ngram_size", 0)
    a.min_length, a.min_new_tokens, a.eos_id = kw.get("min_length", 0), kw.get("min_new_tokens", 0), EOS
    a.n_bad, a.bad_off, a.bad_tok = len(bad), off_d.data_ptr(), tok_d.data_ptr()
    a.out, a.ld_out = out.data_ptr(), V
    a.pick, a.done, a.pad_id, a.tokens, a.stop_word = 1, dd.data_ptr(), 0, tok.data_ptr(), stop.data_ptr()
    if want_logprob:
        a.logprob, a.ld_logprob = lp.data_ptr(), ld_logprob
    L.check(lib.klab_logits_process_rows(C.byref(a), L.stream_ptr()), "klab_logits_process_rows")
    torch.cuda.synchronize()
    return dict(tok=tok.cpu(), out=out.cpu(), done=dd.cpu(), seq=seq_d.cpu(), stop=stop.cpu(), logprob=lp.cpu())


@pytest.mark.parametrize("V", [5, 1000, 32100, 32768])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pick_logprob(V, dtype):
    """4 rows: a live row, a row finished on entry, a row whose largest logit is EOS, and a row of -inf (every score banned)"""
    x = uniform_logits(4, V, dtype, 2000 + V)
    x[2, EOS] = 12.0
    x[3] = -float("inf")
    cur = 6
    hist = torch.randint(0, min(8, V), (4, cur), generator=torch.Generator().manual_seed(V))
    hist[:, 0] = 0
    hist[0, 1:] = torch.tensor([2, 4, 2, 4, 2])  # repeats: the penalty and the n-gram and bad-word bans all bite
    done = torch.tensor([0, 1, 0, 0], dtype=torch.int32)
    for kw in PROC_SETTINGS:
        what = (V, dtype, kw)
        plain = process_pick(x, hist, done, False, **kw)
        got = process_pick(x, hist, done, True, **kw)
        _same_old_outputs(plain, got, what)
        assert (plain["logprob"] == SENTINEL).all(), what
        ref = hf_process(hist, x.float(), **{k: v for k, v in kw.items() if k != "min_new_tokens"},
                         min_new_tokens=kw.get("min_new_tokens")).double()
        assert torch.equal(torch.isinf(got["out"]), torch.isinf(ref)), what
        pick = got["out"].argmax(-1)  # (the kernel's own pick before the pad of the finished row)
        tok = got["tok"]
        assert tok[0] == pick[0] and tok[1] == 0 and tok[2] == pick[2] and tok[3] == 0, (what, tok, pick)
        assert got["done"].tolist() == [int(tok[0] == EOS), 1, int(tok[2] == EOS), 0], what
        if not kw:
            assert int(tok[2]) == EOS, what
        assert (ref.gather(1, pick.view(-1, 1)).squeeze(1) == ref.max(-1)[0]).all(), what
        want = token_logprob(ref, pick)
        lp = got["logprob"]
        assert float(lp[1, cur]) == 0.0, what
        assert float(lp[3, cur]) == -float("inf") and float(want[3]) == -float("inf"), what
        for r in (0, 2):
            assert torch.isfinite(want[r]) and abs(float(lp[r, cur]) - float(want[r])) <= 1e-5, (what, r, float(lp[r, cur]), float(want[r]))
        lp[:, cur] = SENTINEL
        assert (lp == SENTINEL).all(), what


def test_pick_logprob_needs_room():
    x = uniform_logits(1, 5, torch.float32, 1)
    with pytest.raises(ValueError):
        process_pick(x, torch.zeros(1, 3, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), True, ld_logprob=3)


# ---- 3. klab_gen_finalize ------------------------------------------------------------------------------------------------------
def gen_finalize(lp, seq, B, n, length, length_penalty, n_out):
    L, lib = _lib()
    M = B * n
    lpd, sd = lp.cuda(), seq.cuda()
    score = torch.full((M,), float("nan"), device="cuda")
    lens = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    order = torch.full((B * n_out,), -1, dtype=torch.int32, device="cuda")
    L.check(lib.klab_gen_finalize(lpd.data_ptr(), lpd.stride(0), sd.data_ptr(), sd.stride(0), B, n, length, EOS, length_penalty, n_out,
                                  score.data_ptr(), lens.data_ptr(), order.data_ptr(), L.stream_ptr()), "klab_gen_finalize")
    torch.cuda.synchronize()
    return score.cpu(), lens.cpu(), order.cpu()


def finalize_inputs(B, n, length, ld, ld_seq):
    """random log-probabilities and EOS-free sequences, then by hand: row 0 ends at position 1, the first row of image 1 at the
    last position, and (n >= 3) image 1's rows 0 and 1 are equal and its last row holds a -inf; whatever follows an EOS is junk
    that must not count"""
    g = torch.Generator().manual_seed(n)
    M = B * n
    lp = -torch.rand(M, ld, generator=g) * 5.0
    seq = torch.randint(2, 50, (M, ld_seq), generator=g)
    seq[0, 1] = EOS
    lp[0, 2:] = 1000.0
    seq[0, 3] = EOS  # a second EOS after the first changes nothing
    seq[:, length:] = EOS  # beyond `length`: not looked at
    lp[:, length:] = 1000.0
    if B > 1:
        seq[n, length - 1] = EOS
        if n >= 3:
            lp[n + 1], seq[n + 1] = lp[n], seq[n]
            lp[2 * n - 1, 2] = -float("inf")
    return lp, seq


@pytest.mark.parametrize("n", [1, 3, 64])
def test_gen_finalize(n):
    B, length, ld, ld_seq = 2, 6, 8, 7
    lp, seq = finalize_inputs(B, n, length, ld, ld_seq)
    for penalty in (0.0, 1.0, 2.0):
        for n_out in sorted({1, min(2, n), n}):
            what = (n, penalty, n_out)
            score, lens, order = gen_finalize(lp, seq, B, n, length, penalty, n_out)
            wl, ws, wo = sequence_scores(lp.numpy(), seq.numpy(), length, EOS, n, penalty, n_out)
            assert lens.tolist() == wl.tolist(), what
            assert int(lens[0]) == 1 and int(lens[n]) == length - 1, what
            assert order.tolist() == wo.tolist(), what
            fin = np.isfinite(ws)
            assert np.array_equal(np.isinf(score.numpy()), ~fin), what
            assert (np.abs(score.numpy()[fin] - ws[fin]) <= 1e-6 * np.abs(ws[fin])).all(), what
            if n >= 3:
                assert bool(~fin[2 * n - 1]) and int(fin.sum()) == B * n - 1, what
                if n_out == n:
                    o = order.tolist()[n:]
                    assert o[-1] == 2 * n - 1 and o.index(n) + 1 == o.index(n + 1), (what, o)  # -inf last; the tie in row order
            again = gen_finalize(lp, seq, B, n, length, penalty, n_out)
            assert torch.equal(score.view(torch.int32), again[0].view(torch.int32)) and torch.equal(order, again[2]), what


def test_gen_finalize_rejects_more_than_a_wave():
    lp, seq = finalize_inputs(1, 65, 6, 8, 7)
    with pytest.raises(NotImplementedError):
        gen_finalize(lp, seq, 1, 65, 6, 1.0, 1)
    lp, seq = finalize_inputs(1, 3, 6, 8, 7)
    with pytest.raises(ValueError):
        gen_finalize(lp, seq, 1, 3, 6, 1.0, 4)  # n_out > n
    with pytest.raises(ValueError):
        gen_finalize(lp, seq, 1, 3, 9, 1.0, 1)  # length > ld


# ---- the models ------------------------------------------------------------------------------------------------------------------
_ARGS = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                              transformer_model_name="-")


def _build(name, dtype, variant="plain"):
    from klab_multimodalmodel_amd.models.model import MyModel
    if name.startswith("tiny_v11"):
        from tests.v11_helpers import build_v11
        m, g = build_v11(name, dtype, False)
        return m.to("cuda"), g
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    g = load_golden(name)
    sw = SwinConfig.from_dict(g["meta"]["swin_config"])
    t5 = T5Config.from_dict(g["meta"]["t5_config"])
    main = dict(g["sds"]["main"])
    if variant == "eos":
        main["shared.weight"] = main["shared.weight"].clone()
        main["shared.weight"][1] = torch.from_numpy(np.load(os.path.join(GOLD, "beam.npz"))[f"{name}.eos_row"])
    m = MyModel(_ARGS, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], main), dtype=dtype)
    return m.to("cuda"), g


def _inputs(g):
    return g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()


def _live(seq):
    """bool [rows, L - 1]: the generated positions through each row's first EOS"""
    return np.cumsum(np.cumsum(seq[:, 1:] == EOS, 1), 1) <= 1


def _host_scores(lp, seq, penalty):
    live = _live(seq)
    lens = live.sum(1)
    return (np.where(live, lp[:, 1:].astype(np.float64), 0.0).sum(1)) / lens.astype(np.float64) ** penalty, lens


def _session_step_logits(m, pix, src, max_length, mode, n, procs=None, **kw):
    """drives a want_logprobs session by hand: yields (pos, the fp32 logits [B*n, V] position pos was chosen from, eng, ws) after
    every choice"""
    cfg = m.main_cfg
    B = src.shape[0]
    tgt = torch.full((B, max_length - 1), cfg.pad_token_id, dtype=torch.int64, device="cuda")
    eng = m._engine_for(pix, src, tgt)
    m.transformer.eval()
    with torch.no_grad():
        eng.forward(pix, src, tgt, training=0, seed=m._seed_base, want_grad=False)
        first = eng.buffer("logits").view(B, max_length - 1, -1)[:, 0].float().repeat_interleave(n, 0).clone()
        gen = eng.gen_cfg(mode, n, max_length, cfg.eos_token_id, cfg.pad_token_id, procs=procs, want_logprobs=True, **kw)
        ws = torch.empty(eng.gen_workspace_bytes(gen), dtype=torch.uint8, device="cuda")
        eng.gen_begin(gen, ws)
        yield 1, first, eng, ws
        cur = 1
        while cur < max_length - 1 and eng.gen_going(ws, cur):
            eng.gen_step(cur, ws)
            cur += 1
            yield cur, eng.gen_buffer(ws, "logits").float().clone(), eng, ws


# ---- 4. greedy against HF ----------------------------------------------------------------------------------------------------------
# Measured on the MI355X (fp32, the six fixture cases): max |log_softmax(session logits, processed in float64 by torch)[token] -
# fixture| = 1.296e-6 (what the fp32 logits themselves differ from the reference's by); the kernel's own fp32 evaluation order
# is allowed 4x that.  The kernel's column measured 1.431e-6 at most.
YARDSTICK = 1.3e-6
_GOLD = {}


def _gold():
    if not _GOLD:
        _GOLD["z"] = np.load(os.path.join(GOLD, "logprobs.npz"))
        _GOLD["cases"] = json.load(open(os.path.join(GOLD, "logprobs.json")))["cases"]
    return _GOLD["z"], _GOLD["cases"]


def _case_ids():
    return [c["id"] for c in json.load(open(os.path.join(GOLD, "logprobs.json")))["cases"]]


@pytest.mark.parametrize("cid", _case_ids())
def test_generate_greedy_logprobs_match_hf(cid):
    from klab_multimodalmodel_amd.logits_proc import logits_processor_settings
    z, cases = _gold()
    cs = next(c for c in cases if c["id"] == cid)
    m, g = _build(cs["model"], "fp32", cs["variant"])
    pix, src = _inputs(g)
    want_seq, want_lp = z[cid + ".seq"], z[cid + ".logprobs"]
    live = _live(want_seq)
    # the yardstick: torch in float64 on the session's own logits, without the new code
    kw = cs["kwargs"]
    procs = logits_processor_settings(kw.get("repetition_penalty", 1.0), kw.get("no_repeat_ngram_size", 0), None, kw.get("min_length", 0),
                                      None, eos_token_id=m.main_cfg.eos_token_id, vocab_size=m.main_cfg.vocab_size)
    yard = 0.0
    for pos, logits, eng, ws in _session_step_logits(m, pix, src, cs["max_length"], "pick", 1, procs):
        if pos >= want_seq.shape[1]:
            break
        hist = torch.from_numpy(want_seq[:, :pos])
        s = hf_process(hist, logits.cpu(), **kw).double()
        ref = token_logprob(s, torch.from_numpy(want_seq[:, pos]))
        for r in range(want_seq.shape[0]):
            if live[r, pos - 1]:
                yard = max(yard, abs(float(ref[r]) - float(want_lp[r, pos - 1])))
    print(f"{cid}: yardstick (float64 torch on the session logits vs fixture) {yard:.3e}")
    assert yard <= 4 * YARDSTICK, (cid, yard)  # (the session's logits are where they were when the yardstick was taken)
    for penalty in (1.0, 2.0):
        seq, info = m.generate(pix, src, max_length=cs["max_length"], return_logprobs=True, length_penalty=penalty, **kw)
        seq = seq.cpu().numpy()
        assert seq.shape == want_seq.shape and np.array_equal(seq, want_seq), (cid, seq, want_seq)
        lp = info["token_logprobs"].cpu().numpy()
        assert lp.dtype == np.float32 and lp.shape == seq.shape and (lp[:, 0] == 0).all()
        err = float(np.abs(lp[:, 1:][live] - want_lp[live]).max())
        print(f"{cid}: kernel vs fixture {err:.3e}")
        assert err <= 4 * YARDSTICK, (cid, err)
        assert (lp[:, 1:][~live] == 0).all(), cid  # exactly 0 after EOS
        ws_, wl = _host_scores(lp, seq, penalty)
        assert info["lengths"].dtype == torch.int32 and info["lengths"].cpu().tolist() == wl.tolist(), cid
        sc = info["scores"].cpu().numpy().astype(np.float64)
        assert (np.abs(sc - ws_) <= 1e-6 * np.abs(ws_)).all(), (cid, sc, ws_)
    plain = m.generate(pix, src, max_length=cs["max_length"], **kw)
    assert torch.equal(plain.cpu(), torch.from_numpy(want_seq)), cid


# ---- 5. sampling on the model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_generate_sample_logprobs(dtype):
    m, g = _build("tiny_b", dtype)
    pix, src = _inputs(g)
    kw = dict(max_length=12, do_sample=True, num_return_sequences=3, temperature=0.8, top_k=20)
    torch.manual_seed(0)
    plain = m.generate(pix, src, **kw)
    torch.manual_seed(0)
    seq, info = m.generate(pix, src, return_logprobs=True, **kw)
    torch.manual_seed(0)
    seq2, info2 = m.generate(pix, src, return_logprobs=True, **kw)
    assert torch.equal(plain, seq) and torch.equal(seq, seq2)
    for key in ("token_logprobs", "scores"):
        assert torch.equal(info[key].view(torch.int32), info2[key].view(torch.int32)), key
    assert torch.equal(info["lengths"], info2["lengths"])
    lp = info["token_logprobs"].cpu().numpy()
    assert lp.shape == tuple(seq.shape) and (lp[:, 0] == 0).all() and (lp <= 0).all()
    ws_, wl = _host_scores(lp, seq.cpu().numpy(), 1.0)
    assert info["lengths"].cpu().tolist() == wl.tolist()
    assert (np.abs(info["scores"].cpu().numpy() - ws_) <= 1e-6 * np.abs(ws_)).all()
    # by hand: the column written at each step against the restatement on that step's logits
    torch.manual_seed(0)
    seed = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (), dtype=torch.int64))
    worst = 0.0
    for pos, logits, eng, ws in _session_step_logits(m, pix, src, 12, "sample", 3, temperature=0.8, top_k=20, top_p=1.0, seed=seed):
        col = eng.gen_buffer(ws, "logprobs")[:, pos].cpu()
        tok = eng.gen_result(ws, 3, pos + 1)[0][:, pos].cpu()
        assert torch.equal(tok, seq[:, pos].cpu()), pos
        done_before = (seq[:, 1:pos].cpu() == EOS).any(1)
        ref, _ = warped_scores(logits.cpu(), 0.8, 20, 1.0)
        want = token_logprob(ref, tok)
        for r in range(tok.shape[0]):
            if done_before[r]:
                assert float(col[r]) == 0.0
            else:
                worst = max(worst, abs(float(col[r]) - float(want[r])))
        assert torch.equal(col, torch.from_numpy(lp[:, pos])), pos
    print(f"sampling {dtype}: kernel vs float64 restatement {worst:.3e}")
    assert worst <= 1e-5, worst


# ---- 6. best_of ----------------------------------------------------------------------------------------------------------------------
def test_generate_best_of():
    m, g = _build("tiny_b", "fp32")
    pix, src = _inputs(g)
    B = src.shape[0]
    kw = dict(max_length=12, do_sample=True, temperature=0.8, top_k=20)
    torch.manual_seed(3)
    all_seq, all_info = m.generate(pix, src, num_return_sequences=8, return_logprobs=True, **kw)
    torch.manual_seed(3)
    seq, info = m.generate(pix, src, num_return_sequences=2, best_of=8, return_logprobs=True, **kw)
    torch.manual_seed(3)
    only = m.generate(pix, src, num_return_sequences=2, best_of=8, **kw)
    assert torch.equal(only, seq) and seq.shape == (2 * B, all_seq.shape[1])
    sc = all_info["scores"].cpu().numpy()
    rows = []
    for b in range(B):
        rows += sorted(range(b * 8, b * 8 + 8), key=lambda r: (-sc[r], r))[:2]
    assert torch.equal(seq, all_seq[rows])
    for key in ("token_logprobs", "scores", "lengths"):
        assert torch.equal(info[key], all_info[key][rows]), key
    s = info["scores"].cpu().view(B, 2)
    assert (s[:, 0] >= s[:, 1]).all()


def test_gen_session_logprobs_are_optional():
    """a session begun without want_logprobs has no "logprobs" buffer and a workspace smaller by exactly that buffer; beam search
    with want_logprobs is unsupported (0 bytes)"""
    m, g = _build("tiny_b", "fp32")
    pix, src = _inputs(g)
    cfg = m.main_cfg
    B, ml = src.shape[0], 8
    tgt = torch.full((B, ml - 1), cfg.pad_token_id, dtype=torch.int64, device="cuda")
    eng = m._engine_for(pix, src, tgt)
    m.transformer.eval()
    with torch.no_grad():
        eng.forward(pix, src, tgt, training=0, seed=m._seed_base, want_grad=False)
    a = eng.gen_workspace_bytes(eng.gen_cfg("sample", 3, ml, cfg.eos_token_id, cfg.pad_token_id))
    b = eng.gen_workspace_bytes(eng.gen_cfg("sample", 3, ml, cfg.eos_token_id, cfg.pad_token_id, want_logprobs=True))
    assert 0 < a and 0 <= b - a - B * 3 * ml * 4 < 512
    assert eng.gen_workspace_bytes(eng.gen_cfg("beam", 2, ml, cfg.eos_token_id, cfg.pad_token_id, want_logprobs=True)) == 0
    gen = eng.gen_cfg("pick", 1, ml, cfg.eos_token_id, cfg.pad_token_id)
    ws = torch.empty(eng.gen_workspace_bytes(gen), dtype=torch.uint8, device="cuda")
    eng.gen_begin(gen, ws)
    with pytest.raises(KeyError):
        eng.gen_buffer(ws, "logprobs")
    with pytest.raises(ValueError):
        eng.gen_scores(ws, 2)
