"""Forced decoding on the K/V cache: klab_force_rows against the float64 restatement (tests/logprob_ref.py), the force session and
MyModel.score against the session's own logits, the reference's fixture (tests/golden/force.npz from make_force_goldens.py) and
the teacher-forced evaluation forward, generate(decoder_input_ids=...) against HF's sequences, and the sessions without a table
against a model that never arms one."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLD
from tests.logits_proc_ref import hf_process
from tests.logprob_ref import sequence_scores, token_logprob
from tests.sample_ref import hf_warp
from tests.test_logprobs_gpu import _build, _inputs

pytestmark = pytest.mark.gpu

EOS, PAD, START = 1, 0, 0
SEQ_FILL, TOK_FILL = -7, -9


def _lib():
    from klab_multimodalmodel_amd import _lib as L
    return L, L.load()


# ---- 1. klab_force_rows ------------------------------------------------------------------------------------------------------
def force_rows(x, toks, done, pos, row_div, finish, want_logprob, misalign=False, ld=8):
    """one launch over rows = len(toks) rows; x [rows / row_div, V] (host; None: a NULL logits pointer).  logprob, seq and tokens
    have one margin row in front and one behind, the forced table a margin column either side of pos.  misalign: the logits
    start one element off a 16-byte boundary."""
    L, lib = _lib()
    rows = len(toks)
    table = torch.full((rows, ld), 3, dtype=torch.int64)
    if 0 <= pos < ld:
        table[:, pos] = torch.as_tensor(toks)
    td, dd = table.cuda(), torch.as_tensor(done, dtype=torch.int32).cuda()
    lp = torch.full((rows + 2, ld), float("nan"), device="cuda")
    seq = torch.full((rows + 2, ld), SEQ_FILL, dtype=torch.int64, device="cuda")
    tok = torch.full((rows + 2,), TOK_FILL, dtype=torch.int64, device="cuda")
    stop = torch.zeros(3, dtype=torch.int32, device="cuda")
    a = L.ForceArgs()
    if x is not None:
        V = x.shape[1]
        store = torch.zeros(x.numel() + 8, dtype=x.dtype, device="cuda")
        xd = store[1:1 + x.numel()] if misalign else store[:x.numel()]
        xd.copy_(x.reshape(-1))
        assert (xd.data_ptr() % 16 != 0) == misalign
        a.dtype, a.logits, a.ld, a.V = L.dtype_code(x.dtype), xd.data_ptr(), V, V
    a.row_div, a.rows = row_div, rows
    a.forced, a.ld_forced, a.finish_on_eos = td.data_ptr(), ld, finish
    a.done, a.eos_id, a.pad_id, a.start_id = dd.data_ptr(), EOS, PAD, START
    a.tokens, a.seq, a.ld_seq, a.pos, a.stop_word = tok[1:].data_ptr(), seq[1:].data_ptr(), ld, pos, stop[1:].data_ptr()
    if want_logprob:
        a.logprob, a.ld_logprob = lp[1:].data_ptr(), ld
    L.check(lib.klab_force_rows(C.byref(a), L.stream_ptr()), "klab_force_rows")
    torch.cuda.synchronize()
    return dict(tok=tok.cpu(), seq=seq.cpu(), done=dd.cpu(), stop=stop.cpu(), logprob=lp.cpu())


def check_bookkeeping(got, toks, done, pos, finish, what):
    """the restatement of what the two choosing kernels do with a token, and nothing outside the rows / column pos touched"""
    rows = len(toks)
    want_tok = [PAD if d else t for t, d in zip(toks, done)]
    want_done = [int(d or (finish and t == EOS)) for t, d in zip(toks, done)]
    assert got["tok"].tolist() == [TOK_FILL] + want_tok + [TOK_FILL], what
    assert got["done"].tolist() == want_done, what
    assert got["stop"].tolist() == [0, int(not all(want_done)), 0], what
    seq = torch.full((rows + 2, got["seq"].shape[1]), SEQ_FILL, dtype=torch.int64)
    seq[1:-1, pos] = torch.tensor(want_tok)
    if pos == 1:
        seq[1:-1, 0] = START
    assert torch.equal(got["seq"], seq), what


def uniform_logits(rows, V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(rows, V, generator=g) * 24.0 - 12.0).to(dtype)


@pytest.mark.parametrize("V", [5, 1000, 32100, 32768, 40000])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_force_rows_logprob(V, dtype):
    """3 rows, the middle one finished on entry; forced ids 0, V - 1 and EOS among them.  V = 5 takes the scalar path by its
    size, V = 1000 is also run from a misaligned row (scalar path); 40000 is above the register-row kernels' 32768."""
    pos = 3
    done = [0, 1, 0]
    for row_div in (1, 3):
        x = uniform_logits(3 // row_div, V, dtype, 3000 + V + row_div)
        for toks in ([0, 3, V - 1], [EOS, 3, 2]):
            for finish in (0, 1):
                for misalign in ((False, True) if V == 1000 else (False,)):
                    what = (V, dtype, row_div, toks, finish, misalign)
                    got = force_rows(x, toks, done, pos, row_div, finish, True, misalign)
                    check_bookkeeping(got, toks, done, pos, finish, what)
                    want = token_logprob(x.double()[[r // row_div for r in range(3)]], torch.tensor(toks))
                    lp = got["logprob"]
                    assert float(lp[2, pos]) == 0.0, what  # finished on entry: the pad scores 0
                    for r in (0, 2):
                        err = abs(float(lp[1 + r, pos]) - float(want[r]))
                        assert torch.isfinite(want[r]) and err <= 1e-5, (what, r, float(lp[1 + r, pos]), float(want[r]))
                    lp[1:-1, pos] = float("nan")
                    assert torch.isnan(lp).all(), what  # nothing but column pos of the three rows is written
    # one-hot rows: the token's logit 0, every other -1000 -> exactly 0.0
    toks = [0, V - 1, V // 2]
    x = torch.full((3, V), -1000.0, dtype=dtype)
    x[torch.arange(3), torch.tensor(toks)] = 0.0
    got = force_rows(x, toks, [0, 0, 0], pos, 1, 1, True)
    assert got["logprob"][1:-1, pos].tolist() == [0.0, 0.0, 0.0], (V, dtype)


@pytest.mark.parametrize("finish", [0, 1])
def test_force_rows_bookkeeping(finish):
    """done, tokens, seq and the stop word for both values of finish_on_eos, with and without the log-probability; without it the
    logits are never read: a buffer of NaN (and no buffer at all) changes nothing"""
    V = 40
    x = uniform_logits(4, V, torch.float32, 7)
    nan = torch.full((4, V), float("nan"))
    for pos in (1, 4):
        for toks, done in (([EOS, 5, EOS, 39], [0, 0, 1, 1]), ([EOS, EOS, 7, 0], [0, 0, 1, 1]), ([2, EOS, 9, 0], [0, 1, 0, 0])):
            what = (finish, pos, toks, done)
            with_lp = force_rows(x, toks, done, pos, 1, finish, True)
            check_bookkeeping(with_lp, toks, done, pos, finish, what)
            for logits in (x, nan, None):
                got = force_rows(logits, toks, done, pos, 1, finish, False)
                check_bookkeeping(got, toks, done, pos, finish, what)
                assert torch.isnan(got["logprob"]).all(), what
    # every row finished (or finishing): the stop word stays 0 only when EOS finishes a row
    got = force_rows(x, [EOS, EOS, EOS, EOS], [0, 0, 1, 0], 2, 1, finish, True)
    assert got["stop"].tolist() == [0, 1 - finish, 0]


def test_force_rows_bad_arguments():
    x = uniform_logits(3, 8, torch.float32, 1)
    with pytest.raises(ValueError):
        force_rows(x, [0, 1, 2], [0, 0, 0], 8, 1, 1, True)  # pos beyond the table, seq and logprob rows
    with pytest.raises(ValueError):
        force_rows(x, [0, 1, 2], [0, 0, 0], 0, 1, 1, True)  # position 0 is the start token's
    with pytest.raises(ValueError):
        force_rows(None, [0, 1, 2], [0, 0, 0], 3, 1, 1, True)  # a log-probability needs logits
    # a token outside the row reads nothing: -inf (the Python layer refuses such a table first)
    got = force_rows(x, [8, -1, 7], [0, 0, 0], 3, 1, 1, True)
    assert got["logprob"][1:-1, 3].tolist()[:2] == [-float("inf")] * 2 and torch.isfinite(got["logprob"][3, 3])


# ---- the models ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(name, dtype, variant="plain"):
    m, g = _build(name, dtype, variant)
    return m, _inputs(g)


@functools.lru_cache(maxsize=None)
def _gold():
    return np.load(os.path.join(GOLD, "force.npz")), json.load(open(os.path.join(GOLD, "force.json")))


def _live(cand):
    """bool [..., L]: the positions through each row's first EOS"""
    return np.cumsum(cand == EOS, -1) - (cand == EOS) < 1


def _force_session(m, pix, src, cand):
    """a force session driven by hand: (eng, ws, table [M, L + 1] on the host, fp-as-stored logits [M, L, V]: position p + 1 of
    row r was scored on logits[r, p])"""
    cfg = m.main_cfg
    B, N, L = cand.shape
    tgt = torch.full((B, L), cfg.pad_token_id, dtype=torch.int64, device="cuda")
    table = torch.cat([torch.full((B * N, 1), cfg.decoder_start_token_id, dtype=torch.int64), cand.reshape(B * N, L)], 1)
    eng = m._engine_for(pix, src, tgt)
    m.transformer.eval()
    with torch.no_grad():
        eng.forward(pix, src, tgt, training=0, seed=m._seed_base, want_grad=False)
        cols = [eng.buffer("logits").view(B, L, -1)[:, 0].repeat_interleave(N, 0).clone()]
        gen = eng.gen_cfg("force", N, L + 1, cfg.eos_token_id, cfg.pad_token_id, want_logprobs=True)
        ws = torch.empty(eng.gen_workspace_bytes(gen), dtype=torch.uint8, device="cuda")
        eng.gen_set_forced(table.cuda(), L)
        eng.gen_begin(gen, ws)
        for t in range(1, L):
            eng.gen_step(t, ws)
            cols.append(eng.gen_buffer(ws, "logits").clone())
    return eng, ws, table, torch.stack(cols, 1)


def _gathered(logits, cand):
    """float64 log_softmax of logits [M, L, V] at the candidates' tokens, 0 after each row's EOS: [B, N, L]"""
    B, N, L = cand.shape
    lp = torch.log_softmax(logits.double().cpu(), -1).gather(-1, cand.reshape(B * N, L, 1)).view(B, N, L).numpy()
    return np.where(_live(cand.numpy()), lp, 0.0)


def _check_summary(out, cand, penalty, top=None):
    """lengths, scores and order of a score() result against klab_gen_finalize's restatement on its own token_logprobs"""
    B, N, L = cand.shape
    lp = np.concatenate([np.zeros((B * N, 1)), out["token_logprobs"].cpu().numpy().reshape(B * N, L)], 1)
    seq = np.concatenate([np.zeros((B * N, 1), dtype=np.int64), cand.numpy().reshape(B * N, L)], 1)
    wl, wsc, wo = sequence_scores(lp, seq, L + 1, EOS, N, penalty, top or N)
    assert out["lengths"].dtype == torch.int32 and out["lengths"].cpu().view(-1).tolist() == wl.tolist()
    sc = out["scores"].cpu().numpy().astype(np.float64).reshape(-1)
    assert (np.abs(sc - wsc) <= 1e-6 * np.abs(wsc)).all(), (sc, wsc)
    order = out["order"].cpu()
    assert order.dtype == torch.int64 and tuple(order.shape) == (B, top or N)
    assert order.tolist() == (wo.reshape(B, -1) - np.arange(B)[:, None] * N).tolist()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_score_in_place(dtype):
    """every column the session writes against float64 log_softmax of the very logits it was computed from"""
    z, _ = _gold()
    m, (pix, src) = _model("tiny_b", dtype)
    cand = torch.from_numpy(z["tiny_b.plain.cand"])
    B, N, L = cand.shape
    eng, ws, table, logits = _force_session(m, pix, src, cand)
    want = _gathered(logits, cand)
    col = eng.gen_buffer(ws, "logprobs").cpu().numpy()
    assert (col[:, 0] == 0).all()
    err = float(np.abs(col[:, 1:].reshape(B, N, L) - want).max())
    print(f"score in place {dtype}: session vs float64 on its own logits {err:.3e}")
    assert err <= 1e-5, err
    assert torch.equal(eng.gen_result(ws, N, L + 1)[0].cpu()[:, 1:], torch.where(torch.from_numpy(_live(cand.numpy())).view(B * N, L),
                                                                                 table[:, 1:], torch.zeros_like(table[:, 1:])))
    for penalty in (0.0, 1.0, 2.0):
        out = m.score(pix, src, cand, length_penalty=penalty)
        got = out["token_logprobs"].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (B, N, L)
        assert float(np.abs(got - want).max()) <= 1e-5
        assert (got[~_live(cand.numpy())] == 0).all()  # exactly 0 after a row's EOS
        _check_summary(out, cand, penalty)
    _check_summary(m.score(pix, src, cand.cuda(), length_penalty=1.0, top=2), cand, 1.0, top=2)


@pytest.mark.parametrize("mid", ["tiny_b.plain", "tiny_b.eos", "tiny_v11_a.plain"])
def test_score_matches_the_reference(mid):
    """fp32 engine against the reference's float64 log-probabilities of the same candidates.  The yardstick -- what the engine's
    fp32 logits themselves differ from the reference's by, taken with torch in float64 on the session's own logits -- measured
    8.5e-7 to 9.3e-7 over the three models on the MI355X, the kernel's column 1.37e-6 at most; the kernel's
    column is allowed 4x the yardstick of its own run."""
    z, _ = _gold()
    name, variant = mid.rsplit(".", 1)
    m, (pix, src) = _model(name, "fp32", variant)
    cand = torch.from_numpy(z[mid + ".cand"])
    live = _live(cand.numpy())
    fix = z[mid + ".cand_logprobs"]
    _, _, _, logits = _force_session(m, pix, src, cand)
    yard = float(np.abs(_gathered(logits, cand) - fix)[live].max())
    for penalty in (0, 1):
        out = m.score(pix, src, cand, length_penalty=float(penalty))
        err = float(np.abs(out["token_logprobs"].cpu().numpy() - fix)[live].max())
        print(f"{mid}: yardstick {yard:.3e}, score vs fixture {err:.3e}")
        assert err <= 4 * yard, (mid, err, yard)
        order = out["order"].cpu().numpy()
        assert np.array_equal(order, z[mid + f".cand_order{penalty}"]), (mid, penalty)
        top2 = m.score(pix, src, cand, length_penalty=float(penalty), top=2)["order"].cpu().numpy()
        assert np.array_equal(top2, order[:, :2])


def test_score_matches_the_evaluation_forward():
    """the only other way to score: one teacher-forced evaluation forward with the images replicated N times"""
    z, _ = _gold()
    m, (pix, src) = _model("tiny_b", "fp32")
    cand = torch.from_numpy(z["tiny_b.plain.cand"]).clone()
    cand[:, 4] = cand[:, 3]  # row 4 = row 3 padded after its EOS instead of the junk
    cand[:, 4, 3:] = PAD
    B, N, L = cand.shape
    live = _live(cand.numpy())
    assert (cand[:, 3, 3:] > 1).all() and live[:, 3].sum() == live[:, 4].sum() == 3 * B
    _, _, table, logits = _force_session(m, pix, src, cand)
    ours = _gathered(logits, cand)
    pr, sr, tgt = pix.repeat_interleave(N, 0).contiguous(), src.repeat_interleave(N, 0).contiguous(), table[:, 1:].contiguous().cuda()
    eng = m._engine_for(pr, sr, tgt)
    eng.forward(pr, sr, tgt, training=0, seed=0, want_grad=False)
    fwd = _gathered(eng.buffer("logits").view(B * N, L, -1).clone(), cand)
    d0 = float(np.abs(fwd - ours).max())
    out = m.score(pix, src, cand, length_penalty=0.0)
    got = out["token_logprobs"].cpu().numpy()
    err = float(np.abs(got - fwd).max())
    print(f"evaluation forward vs session logits d0 {d0:.3e}; score vs evaluation forward {err:.3e}")
    assert err <= d0 + 1e-5, (err, d0)
    total = np.where(live, fwd, 0.0).sum(-1)
    assert (np.abs(out["scores"].cpu().numpy() - total) <= L * (d0 + 1e-5)).all()
    # junk after the EOS counts for nothing
    assert np.array_equal(got[:, 3].view(np.int32), got[:, 4].view(np.int32))
    assert torch.equal(out["scores"][:, 3].view(torch.int32), out["scores"][:, 4].view(torch.int32))
    assert torch.equal(out["lengths"][:, 3], out["lengths"][:, 4])
    order = out["order"].cpu().tolist()
    assert all(o.index(3) + 1 == o.index(4) for o in order)  # the tie in candidate order


# ---- decoder prompts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mid", ["tiny_b.plain", "tiny_b.eos", "tiny_v11_a.plain"])
def test_generate_with_a_decoder_prompt_matches_hf(mid):
    z, meta = _gold()
    name, variant = mid.rsplit(".", 1)
    m, (pix, src) = _model(name, "fp32", variant)
    cases = [c for c in meta["cases"] if c["id"].startswith(mid + ".")]
    assert len(cases) == 6
    for cs in cases:
        prompt, want = torch.from_numpy(z[cs["id"] + ".prompt"]), torch.from_numpy(z[cs["id"] + ".seq"])
        got = m.generate(pix, src, max_length=cs["max_length"], decoder_input_ids=prompt.cuda(), **cs["kwargs"]).cpu()
        assert got.shape == want.shape and torch.equal(got, want), (cs["id"], got, want)
        # the start token given explicitly in every row is not prepended again
        with_start = torch.cat([torch.zeros(len(prompt), 1, dtype=torch.int64), prompt], 1)
        assert torch.equal(m.generate(pix, src, max_length=cs["max_length"], decoder_input_ids=with_start, **cs["kwargs"]).cpu(), want)
    # a prompt that is the start token alone is today's call, bit for bit
    plain = m.generate(pix, src, max_length=10)
    assert torch.equal(m.generate(pix, src, max_length=10, decoder_input_ids=torch.zeros(len(prompt), 1, dtype=torch.int64)), plain)
    # a row whose prompt holds an EOS keeps generating
    cs = next(c for c in cases if c["id"].endswith("p3.minnew"))
    got = m.generate(pix, src, max_length=10, decoder_input_ids=torch.from_numpy(z[cs["id"] + ".prompt"]), min_new_tokens=3).cpu()
    assert (got[:, 1:4] == EOS).any(1).all() and (got[:, 4:7] > 1).all()


def test_sample_with_a_decoder_prompt():
    z, _ = _gold()
    m, (pix, src) = _model("tiny_b", "fp32")
    prompt = torch.from_numpy(z["tiny_b.plain.p3.none.prompt"])
    B, P = prompt.shape
    n, ml, temp, k, mnt = 3, 10, 0.8, 20, 3
    procs = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    kw = dict(max_length=ml, do_sample=True, num_return_sequences=n, temperature=temp, top_k=k, min_new_tokens=mnt,
              decoder_input_ids=prompt, **procs)
    torch.manual_seed(5)
    seq = m.generate(pix, src, **kw).cpu()
    torch.manual_seed(5)
    assert torch.equal(m.generate(pix, src, **kw).cpu(), seq)
    assert seq.shape[0] == B * n and (seq[:, 0] == START).all()
    assert torch.equal(seq[:, 1:1 + P], prompt.repeat_interleave(n, 0))  # the prompt columns are exact, EOS included
    assert (seq[:, 1:1 + P] == EOS).any(1).all() and (seq[:, 1 + P:1 + P + mnt] != EOS).all()  # ... and the rows keep generating
    # every later token lies in HF's kept set of its teacher-forced processed logits
    tgt = seq[:, 1:].contiguous().cuda()
    pr, sr = pix.repeat_interleave(n, 0).contiguous(), src.repeat_interleave(n, 0).contiguous()
    eng = m._engine_for(pr, sr, tgt)
    eng.forward(pr, sr, tgt, training=0, seed=0, want_grad=False)
    lg = eng.buffer("logits").view(tgt.shape[0], tgt.shape[1], -1).float().cpu()
    Lp = 1 + P
    done = torch.zeros(B * n, dtype=torch.bool)
    for t in range(Lp, seq.shape[1]):  # position t is chosen from the history seq[:, :t]
        # HF: min_length = min_new_tokens + Lp; EOS banned while t - Lp < min_new_tokens, i.e. t - 1 < min_new_tokens + Lp - 1
        s = hf_process(seq[:, :t], lg[:, t - 1], min_length=mnt + Lp, min_new_tokens=mnt + Lp - 1, **procs)
        kept = ~torch.isinf(hf_warp(s, temp, k, 1.0))
        inside = kept.gather(1, seq[:, t:t + 1]).squeeze(1)
        assert inside[~done].all(), t
        assert (seq[done, t] == PAD).all(), t
        done |= seq[:, t] == EOS


# ---- sessions without a table ----------------------------------------------------------------------------------------------------
def test_sessions_without_a_table_are_unchanged():
    """a model that armed tables (refused, consumed) decodes bit-equal to one that never called the entry point"""
    ma, (pix, src) = _model("tiny_b", "fp32")
    mb, _ = _build("tiny_b", "fp32")
    cfg = ma.main_cfg
    B, ml = src.shape[0], 10
    tgt = torch.full((B, ml - 1), cfg.pad_token_id, dtype=torch.int64, device="cuda")
    table = torch.full((B * 2, ml), 5, dtype=torch.int64, device="cuda")
    sizes = []
    for m in (ma, mb):
        eng = m._engine_for(pix, src, tgt)
        m.transformer.eval()
        with torch.no_grad():
            eng.forward(pix, src, tgt, training=0, seed=m._seed_base, want_grad=False)
        if m is ma:
            beam = eng.gen_cfg("beam", 2, ml, cfg.eos_token_id, cfg.eos_token_id)
            ws = torch.empty(eng.gen_workspace_bytes(beam), dtype=torch.uint8, device="cuda")
            eng.gen_set_forced(table, 3)
            with pytest.raises(ValueError):
                eng.gen_begin(beam, ws)  # beam search takes no forced tokens
            eng.gen_begin(beam, ws)  # ... and the refused begin left nothing armed
            with pytest.raises(ValueError):
                eng.gen_set_forced(table, ml)  # no room for position ml
            force = eng.gen_cfg("force", 2, ml, cfg.eos_token_id, cfg.pad_token_id, want_logprobs=True)
            with pytest.raises(ValueError):
                eng.gen_begin(force, ws)  # a force session needs its table
            eng.gen_set_forced(table, 3)
            with pytest.raises(ValueError):
                eng.gen_begin(force, ws)  # ... for every position
            assert eng.gen_workspace_bytes(eng.gen_cfg("force", 2, ml, cfg.eos_token_id, cfg.pad_token_id)) == 0  # want_logprobs is required
            assert eng.gen_workspace_bytes(force) == eng.gen_workspace_bytes(
                eng.gen_cfg("pick", 2, ml, cfg.eos_token_id, cfg.pad_token_id, want_logprobs=True))
        sizes.append([eng.gen_workspace_bytes(eng.gen_cfg(mode, 2, ml, cfg.eos_token_id, cfg.pad_token_id, want_logprobs=lp))
                      for mode, lp in (("pick", False), ("pick", True), ("sample", False), ("sample", True), ("beam", False))])
    assert sizes[0] == sizes[1] and all(s > 0 for s in sizes[0])
    outs = []
    for m in (ma, mb):
        torch.manual_seed(11)
        o = [m.generate(pix, src, max_length=ml), m.generate(pix, src, max_length=ml, repetition_penalty=1.3, no_repeat_ngram_size=2)]
        o += list(m.generate(pix, src, max_length=ml, num_beams=3, num_return_sequences=2, return_scores=True))
        s, info = m.generate(pix, src, max_length=ml, do_sample=True, num_return_sequences=3, top_k=20, return_logprobs=True)
        o += [s, info["token_logprobs"], info["scores"], info["lengths"]]
        outs.append(o)
    for a, b in zip(*outs):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                         b.view(torch.int32) if b.dtype == torch.float32 else b)
