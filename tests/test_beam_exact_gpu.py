"""The entry points of csrc/beam.hip against tests/beam_ref.py: `klab_beam_topk_scores` bit for bit (scores and flat indices, ties
included) at every list length the row kernel is instantiated with, both load loops, shared rows and unaligned layouts;
`klab_beam_topk` with exact indices and the existing test's score tolerance; `klab_beam_update` single steps and whole scripted
searches (init, top-k, update with the engine's ping-pong buffers) bit for bit; `klab_beam_init`; `klab_beam_copy_rows`.
tests/test_decode_select_fixtures_cpu.py proves the fixtures are what this file takes them for."""
import ctypes as C

import pytest
import torch

from tests import beam_ref as R

pytestmark = pytest.mark.gpu

B = R.B
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _lib():
    from klab_multimodalmodel_amd import _lib as L
    return L, L.load()


def _on_device(x, V, lay, gap):
    """x [rows, V] in the layout `lay` on the device, the gap columns and the buffer's ends holding `gap`: (keep-alive buffer, view)"""
    ld, off = R.layout(lay, V)
    buf, _ = R.device_layout(x, ld, off, gap)
    buf = buf.cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, buf[off:off + x.shape[0] * ld].view(x.shape[0], ld)


def _topk(entry, view, row_div, rs, k, V):
    L, lib = _lib()
    K2 = 2 * k
    rsc = torch.full((B * k, K2), float("nan"), device="cuda")
    ri = torch.full((B * k, K2), -5, dtype=torch.int32, device="cuda")
    osc = torch.full((B, K2), float("nan"), device="cuda")
    oi = torch.full((B, K2), -5, dtype=torch.int32, device="cuda")
    rs_d = rs.cuda().contiguous()
    tail = (rs_d.data_ptr(), B, k, V, rsc.data_ptr(), ri.data_ptr(), osc.data_ptr(), oi.data_ptr(), L.stream_ptr())
    if entry == "scores":
        rc = lib.klab_beam_topk_scores(view.data_ptr(), view.stride(0), row_div, *tail)
    else:
        rc = lib.klab_beam_topk(L.dtype_code(view.dtype), view.data_ptr(), view.stride(0), row_div, *tail)
    L.check(rc, entry)
    torch.cuda.synchronize()
    return osc.cpu(), oi.cpu().long()


# ---- klab_beam_topk_scores: bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.KS)
def test_topk_scores_exact(k):
    for V in R.vocabs(k):
        for lay in R.LAYOUTS:
            for kind in R.SCORE_KINDS:
                x, rs = R.scores_fixture(kind, k, V, lay)
                _buf, view = _on_device(x, V, lay, float("inf"))
                got_s, got_i = _topk("scores", view, 1, rs, k, V)
                want_s, want_i = R.topk_reference(x, rs, k, V, 1, True)
                what = (k, V, lay, kind)
                assert torch.equal(got_i, want_i), (what, got_i, want_i)
                assert torch.equal(got_s, want_s), (what, got_s, want_s)
                assert int(got_i.max()) < k * V, what  # V >= 2k: the list's (-inf, INT_MAX) sentinel never comes back


# ---- klab_beam_topk: exact indices, the existing test's score tolerance -----------------------------------------------------------------
@pytest.mark.parametrize("dn", ["f32", "bf16"])
@pytest.mark.parametrize("k", R.KS)
def test_topk_logits_indices_exact(k, dn):
    dtype = DT[dn]
    for V in R.vocabs(k):
        for lay in R.LAYOUTS:
            for row_div in sorted({1, k}):
                for kind, tie_rows in [(kd, False) for kd in R.LOGIT_KINDS] + ([("b", True)] if row_div > 1 else []):
                    x, rs = R.logits_fixture(kind, k, V, row_div, dn, lay, tie_rows)
                    _buf, view = _on_device(x.to(dtype), V, lay, 1.0e4)
                    got_s, got_i = _topk("logits", view, row_div, rs, k, V)
                    want_s, want_i = R.topk_reference(x.float(), rs, k, V, row_div, False)
                    what = (k, dn, V, lay, row_div, kind, tie_rows)
                    assert torch.equal(got_i, want_i), (what, got_i, want_i)
                    ulp = torch.nextafter(want_s.abs(), torch.tensor(float("inf"))) - want_s.abs()
                    err = (got_s - want_s).abs()
                    assert bool((err <= 1e-5 + ulp).all()), (what, float(err.max()))


def test_topk_argument_checks():
    L, lib = _lib()
    x = torch.zeros(4 * 17, 64, device="cuda")
    rs = torch.zeros(4, 17, device="cuda")
    o = [torch.zeros(4 * 17 * 34, device="cuda") for _ in range(2)]
    oi = [torch.zeros(4 * 17 * 34, dtype=torch.int32, device="cuda") for _ in range(2)]
    for k, V, ld in ((17, 64, 64), (4, 7, 64), (4, 16, 15)):
        tail = (rs.data_ptr(), 4, k, V, o[0].data_ptr(), oi[0].data_ptr(), o[1].data_ptr(), oi[1].data_ptr(), L.stream_ptr())
        assert lib.klab_beam_topk(L.F32, x.data_ptr(), ld, 1, *tail) == L.ERR_BADARG, (k, V, ld)
        assert lib.klab_beam_topk_scores(x.data_ptr(), ld, 1, *tail) == L.ERR_BADARG, (k, V, ld)


# ---- klab_beam_update --------------------------------------------------------------------------------------------------------------------
class _Dev:
    """the device side of a beam state: two parities of the sequence and slot buffers, the scalars, and the argument struct of step c"""

    def __init__(self, k, V, Lm, eos, es, lp, slots=True):
        self.k, self.V, self.Lm, self.cfg = k, V, Lm, (eos, es, lp)
        n = B * k
        self.run_seq = [torch.full((B, k, Lm), -1, dtype=torch.int64, device="cuda") for _ in range(2)]
        self.fin_seq = [torch.full((B, k, Lm), -1, dtype=torch.int64, device="cuda") for _ in range(2)]
        self.slot = [torch.full((n, Lm), -1, dtype=torch.int32, device="cuda") for _ in range(2)] if slots else None
        self.run_score = torch.full((B, k), float("nan"), device="cuda")
        self.fin_score = torch.full((B, k), float("nan"), device="cuda")
        self.fin_flag = torch.full((B, k), -1, dtype=torch.int32, device="cuda")
        self.fin_len = torch.full((B, k), -1, dtype=torch.int32, device="cuda")
        self.unsat = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        self.prev = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        self.parent = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.stop = torch.full((Lm,), -1, dtype=torch.int32, device="cuda")
        self.cand_score = torch.empty(B, 2 * k, device="cuda")
        self.cand_idx = torch.empty(B, 2 * k, dtype=torch.int32, device="cuda")
        self.row_score = torch.empty(n, 2 * k, device="cuda")
        self.row_idx = torch.empty(n, 2 * k, dtype=torch.int32, device="cuda")

    def load(self, st, c):
        """the host state st as the input of step c"""
        i = (c + 1) & 1
        self.run_seq[i].copy_(st["run_seq"])
        self.fin_seq[i].copy_(st["fin_seq"])
        self.fin_score.copy_(st["fin_score"])
        self.fin_flag.copy_(st["fin_flag"].int())
        self.fin_len.copy_(st["fin_len"])
        self.unsat.copy_(st["unsat"].view(-1).int())
        self.stop.zero_()
        if self.slot:
            self.slot[i].copy_(st["slot"])

    def args(self, c):
        L, _ = _lib()
        eos, es, lp = self.cfg
        i, o = (c + 1) & 1, c & 1
        return L.BeamUpdateArgs(B, self.k, self.V, self.Lm, eos, es, lp, self.cand_score.data_ptr(), self.cand_idx.data_ptr(),
                                self.run_seq[i].data_ptr(), self.run_seq[o].data_ptr(), self.run_score.data_ptr(),
                                self.fin_seq[i].data_ptr(), self.fin_seq[o].data_ptr(), self.fin_score.data_ptr(), self.fin_flag.data_ptr(),
                                self.fin_len.data_ptr(), self.unsat.data_ptr(), self.slot[i].data_ptr() if self.slot else None,
                                self.slot[o].data_ptr() if self.slot else None, self.prev.data_ptr(), self.parent.data_ptr(),
                                self.stop.data_ptr())

    def update(self, c):
        L, lib = _lib()
        a = self.args(c)
        L.check(lib.klab_beam_update(C.byref(a), c, L.stream_ptr()), "klab_beam_update")
        torch.cuda.synchronize()

    def state(self, c):
        """what step c (or klab_beam_init, c = 0: the buffers step 1 reads) left, in update_reference's names, on the host"""
        o = c & 1
        k = self.k
        rows = self.parent.cpu().long()
        out = dict(run_seq=self.run_seq[o].cpu(), fin_seq=self.fin_seq[o].cpu(), run_score=self.run_score.cpu(),
                   fin_score=self.fin_score.cpu(), fin_flag=self.fin_flag.cpu().bool(), fin_len=self.fin_len.cpu(),
                   unsat=self.unsat.cpu().bool().view(B, 1), tok=self.prev.cpu().view(B, k), rows=rows,
                   par=rows.view(B, k) - torch.arange(B)[:, None] * k, stop=self.stop.cpu(), word=int(self.stop[c]) if c else 0)
        if self.slot:
            out["slot"] = self.slot[o].cpu()
        return out


@pytest.mark.parametrize("Lm", [8, 70])
@pytest.mark.parametrize("k", R.UPDATE_KS)
def test_update_single_steps(k, Lm):
    V, eos = R.UPDATE_V, R.EOS
    g = torch.Generator().manual_seed(100 * k + Lm)
    for es in (0, 1, 2):
        for lp in (1.0, 0.0, 2.0):
            cfg = dict(k=k, V=V, Lm=Lm, eos=eos, lp=lp, es=es)
            devs = [_Dev(k, V, Lm, eos, es, lp, slots=True), _Dev(k, V, Lm, eos, es, lp, slots=False)]
            for c in R.update_steps(Lm):
                for full, unsat, eos_at in R.SCENARIOS:
                    st = R.random_state(B, k, Lm, g, c, full, unsat)
                    st["slot"] = (torch.arange(B * k * Lm, dtype=torch.int32).view(B * k, Lm) * 5 + c) % (B * k)
                    cs, ci = R.random_candidates(B, k, V, g, eos_at(k))
                    want = R.update_reference(st, cs, ci, c, cfg)
                    what = (k, Lm, es, lp, c, full, unsat, eos_at(k))
                    got = []
                    for d in devs:
                        d.load(st, c)
                        d.cand_score.copy_(cs)
                        d.cand_idx.copy_(ci.int())
                        d.update(c)
                        got.append(d.state(c))
                    rows = got[0]["rows"]
                    want["slot"] = st["slot"][rows].clone()
                    want["slot"][:, c] = torch.arange(B * k, dtype=torch.int32)
                    assert R.state_mismatches(got[0], want, c) == [], what
                    assert R.state_mismatches(got[1], want, c, slot=False) == [], what
                    for n in ("run_seq", "fin_seq", "fin_len", "stop"):  # without the slot table: everything else the same
                        assert torch.equal(got[0][n], got[1][n]), (what, n)


@pytest.mark.parametrize("lp", [0.0, 1.0])
@pytest.mark.parametrize("k", [2, 3, 8, 16])
def test_update_exact_ties(k, lp):
    V, Lm, eos = R.UPDATE_V, 8, R.EOS
    g = torch.Generator().manual_seed(7 * k)
    for es in (0, 1, 2):
        for c in (2, 3, 5):
            cfg = dict(k=k, V=V, Lm=Lm, eos=eos, lp=lp, es=es)
            st, cs, ci = R.tie_scenario(k, Lm, c, lp, g)
            st["slot"] = torch.arange(B * k * Lm, dtype=torch.int32).view(B * k, Lm) % (B * k)
            want = R.update_reference(st, cs, ci, c, cfg)
            d = _Dev(k, V, Lm, eos, es, lp)
            d.load(st, c)
            d.cand_score.copy_(cs)
            d.cand_idx.copy_(ci.int())
            d.update(c)
            got = d.state(c)
            want["slot"] = st["slot"][got["rows"]].clone()
            want["slot"][:, c] = torch.arange(B * k, dtype=torch.int32)
            assert R.state_mismatches(got, want, c) == [], (k, lp, es, c)


# ---- klab_beam_init, klab_beam_topk_scores and klab_beam_update chained as the engine chains them -------------------------------------------
@pytest.mark.parametrize("k,V,Lm", R.SEARCHES)
def test_scripted_search(k, V, Lm):
    L, lib = _lib()
    score_fn = R.scripted_scores(k, V, Lm)
    dev_scores = {}
    for es in R.SEARCH_ES:
        for lp in R.SEARCH_LP:
            cfg = dict(k=k, V=V, Lm=Lm, eos=R.EOS, lp=lp, es=es)
            want = R.search_reference(score_fn, B, k, V, Lm, cfg)
            d = _Dev(k, V, Lm, R.EOS, es, lp)
            a = d.args(1)
            L.check(lib.klab_beam_init(C.byref(a), R.START, R.FILL, L.stream_ptr()), "klab_beam_init")
            torch.cuda.synchronize()
            got = d.state(0)
            for n in ("run_seq", "fin_seq", "run_score", "fin_score", "fin_flag", "fin_len", "unsat", "stop"):
                assert torch.equal(got[n], want[0][n]), (k, es, lp, "init", n)
            assert torch.equal(got["slot"][:, 0], want[0]["slot"][:, 0]), (k, es, lp, "init slot")
            for w in want[1:]:
                c = w["c"]
                if c not in dev_scores:
                    dev_scores[c] = score_fn(c).cuda()
                x = dev_scores[c]
                L.check(lib.klab_beam_topk_scores(x.data_ptr(), V, 1, d.run_score.data_ptr(), B, k, V, d.row_score.data_ptr(),
                                                  d.row_idx.data_ptr(), d.cand_score.data_ptr(), d.cand_idx.data_ptr(), L.stream_ptr()),
                        "klab_beam_topk_scores")
                d.update(c)
                got = d.state(c)
                what = (k, V, Lm, es, lp, c)
                assert torch.equal(d.cand_score.cpu(), w["cand_score"]) and torch.equal(d.cand_idx.cpu().long(), w["cand_idx"]), what
                assert R.state_mismatches(got, w, c) == [], what
                assert torch.equal(got["stop"][:c + 1], w["stop"][:c + 1]), what  # the reference ends the search: same word, same end


# ---- klab_beam_copy_rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem_bytes", [2, 4, 8])
def test_copy_rows(elem_bytes):
    L, lib = _lib()
    dt = {2: torch.int16, 4: torch.int32, 8: torch.int64}[elem_bytes]
    rows = 7
    g = torch.Generator().manual_seed(elem_bytes)
    for src_div in (1, 3):
        for cols in (1, 255, 256, 257, 1000):
            src_ld, dst_ld = cols + 5, cols + 2
            n_src = (rows + src_div - 1) // src_div
            src = torch.randint(-30000, 30000, (n_src, src_ld), generator=g).to(dt)
            dst = torch.full((rows, dst_ld), -77, dtype=dt, device="cuda")
            src_d = src.cuda()
            L.check(lib.klab_beam_copy_rows(elem_bytes, src_d.data_ptr(), src_ld, src_div, dst.data_ptr(), dst_ld, rows, cols, L.stream_ptr()),
                    "klab_beam_copy_rows")
            torch.cuda.synchronize()
            want = torch.full((rows, dst_ld), -77, dtype=dt)
            want[:, :cols] = src[torch.arange(rows) // src_div, :cols]
            assert torch.equal(dst.cpu(), want), (elem_bytes, src_div, cols)
    x = torch.zeros(8, 8, dtype=torch.int32, device="cuda")
    assert lib.klab_beam_copy_rows(3, x.data_ptr(), 8, 1, x.data_ptr(), 8, 1, 1, L.stream_ptr()) == L.ERR_BADARG
