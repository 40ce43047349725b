"""klab_logits_process_rows (csrc/logits_proc.hip) against tests/logits_proc_ref.py's process_reference: bit for bit without
log_softmax (one IEEE multiply or divide per penalised score, -inf per ban), the -inf pattern exact and the finite values within
the existing test's tolerance of the fp64 log_softmax with it.  Histories reach every bitmap word, the partial last word, ids
outside the vocabulary and the history limit; vocabularies and layouts take the scalar and the vector load and store loops.
tests/test_decode_select_fixtures_cpu.py proves the fixtures are what this file takes them for."""
import ctypes as C

import pytest
import torch

from tests import logits_proc_ref as P

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")


def _lib():
    from klab_multimodalmodel_amd import _lib as L
    return L, L.load()


def _tables(bad_words_ids):
    off = [0]
    for w in bad_words_ids:
        off.append(off[-1] + len(w))
    return (torch.tensor(off, dtype=torch.int32, device="cuda"),
            torch.tensor([t for w in bad_words_ids for t in w] or [0], dtype=torch.int32, device="cuda"))


def run(x, hist, V, row_div, odd, log_softmax, pick, kw, tables):
    """the kernel over x [R, V] (host, its dtype) with histories hist; aligned: ld = ld_out = V; odd: ld = V + 3 and ld_out = V + 1
    from bases one element past an aligned address.  Returns (out [rows, V], the gap columns and ends of the out buffer, tokens)."""
    L, lib = _lib()
    rows, cur = hist.shape
    R = x.shape[0]
    ld, ld_out, off = (V + 3, V + 1, 1) if odd else (V, V, 0)
    xb = torch.full((off + R * ld + 8,), 50.0, dtype=x.dtype)
    xb[off:off + R * ld].view(R, ld)[:, :V] = x
    xb = xb.cuda()
    ob = torch.full((off + rows * ld_out + 8,), NAN, device="cuda")
    seq = torch.zeros(rows, cur + 1, dtype=torch.int64)
    seq[:, :cur] = hist
    seq[:, 0] = -9  # position 0 is the start token whatever the buffer holds
    seq_d = seq.cuda()
    tok = torch.full((rows,), -1, dtype=torch.int64, device="cuda")
    stop = torch.zeros(1, dtype=torch.int32, device="cuda")
    a = L.LogitsProcArgs()
    a.dtype, a.logits, a.ld, a.row_div, a.rows, a.V = L.dtype_code(x.dtype), xb.data_ptr() + off * x.element_size(), ld, row_div, rows, V
    a.log_softmax, a.seq, a.ld_seq, a.cur_len, a.start_id = int(log_softmax), seq_d.data_ptr(), cur + 1, cur, 0
    a.repetition_penalty, a.no_repeat_ngram_size = kw.get("repetition_penalty", 1.0), kw.get("no_repeat_ngram_size", 0)
    a.min_length, a.min_new_tokens, a.eos_id = kw.get("min_length", 0), kw.get("min_new_tokens", 0), P.EOS
    a.n_bad, a.bad_off, a.bad_tok = len(kw.get("bad_words_ids", ())), tables[0].data_ptr(), tables[1].data_ptr()
    a.out, a.ld_out = ob.data_ptr() + off * 4, ld_out
    if pick:
        a.pick, a.tokens, a.stop_word = 1, tok.data_ptr(), stop.data_ptr()
    rc = lib.klab_logits_process_rows(C.byref(a), L.stream_ptr())
    L.check(rc, "klab_logits_process_rows")
    torch.cuda.synchronize()
    ob = ob.cpu()
    view = ob[off:off + rows * ld_out].view(rows, ld_out)
    gaps = torch.cat((ob[:off], view[:, V:].reshape(-1), ob[off + rows * ld_out:]))
    return view[:, :V].clone(), gaps, tok.cpu()


@pytest.mark.parametrize("dn", ["f32", "bf16"])
@pytest.mark.parametrize("V", P.PROC_VOCABS)
def test_process_rows_exact(V, dn):
    dtype = DT[dn]
    settings = P.proc_settings(V)
    tables = [_tables(kw.get("bad_words_ids", ())) for kw in settings]
    for row_div in (1, 3):
        for cur in P.PROC_CUR:
            x, hist = P.proc_fixture(V, row_div, cur)
            x32 = x.float().repeat_interleave(row_div, 0)
            for si, kw in enumerate(settings):
                for log_softmax in (False, True):
                    odd = (si + cur + int(log_softmax) + row_div) % 2 == 1  # both layouts under every setting, cur_len and form
                    want = P.process_reference(hist, x32, V, log_softmax=log_softmax, **kw)
                    got, gaps, tok = run(x.to(dtype), hist, V, row_div, odd, log_softmax, True, kw, tables[si])
                    what = (V, dn, row_div, cur, si, log_softmax, odd)
                    assert bool(torch.isnan(gaps).all()), what  # nothing written past V
                    if not log_softmax:
                        assert torch.equal(got, want), (what, torch.nonzero(got != want)[:8])
                    else:
                        assert torch.equal(torch.isinf(got), torch.isinf(want)) and not torch.isnan(got).any(), what
                        fin = ~torch.isinf(want)
                        # fp64 log_softmax rounded to f32, then the f32 penalty: the existing test's tolerance
                        assert torch.allclose(got[fin], want[fin], rtol=1e-6, atol=2e-6), (what, float((got[fin] - want[fin]).abs().max()))
                    first_max = (got == got.max(-1, keepdim=True)[0]).int().argmax(-1)
                    assert torch.equal(tok, first_max), (what, tok, first_max)


def test_process_rows_pick_ties_across_waves():
    """row 0 of the fixture ties exactly at the maximum between two tokens that different waves own: the lower id is picked, and
    the higher one once the lower is banned"""
    V = 32768
    x, hist = P.proc_fixture(V, 1, 3)
    lo, hi = P.tie_tokens(V)
    assert lo // 2048 != hi // 2048
    for dn in ("f32", "bf16"):
        for kw, want in ((dict(), lo), (dict(bad_words_ids=[[lo]]), hi)):
            got, _, tok = run(x.to(DT[dn]), hist, V, 1, False, False, True, kw, _tables(kw.get("bad_words_ids", ())))
            assert int(tok[0]) == want and float(got[0, hi]) == 9.0, (dn, kw, tok)


def test_process_rows_history_limit():
    L, lib = _lib()
    x = torch.zeros(1, 64, device="cuda")
    seq = torch.zeros(1, 1026, dtype=torch.int64, device="cuda")
    out = torch.zeros(1, 64, device="cuda")
    a = L.LogitsProcArgs()
    a.dtype, a.logits, a.ld, a.row_div, a.rows, a.V = L.F32, x.data_ptr(), 64, 1, 1, 64
    a.seq, a.ld_seq, a.cur_len, a.repetition_penalty, a.out, a.ld_out = seq.data_ptr(), 1026, 1025, 1.0, out.data_ptr(), 64
    assert lib.klab_logits_process_rows(C.byref(a), L.stream_ptr()) == L.ERR_UNSUPPORTED
    a.cur_len = 1024
    assert lib.klab_logits_process_rows(C.byref(a), L.stream_ptr()) == 0
    torch.cuda.synchronize()
