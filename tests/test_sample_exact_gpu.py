"""klab_sample_rows (csrc/sample.hip) with no allowance, on tests/sample_ref.py's tie-group fixture: the kept set equals the kernel's
stated rule (kept_reference, fp64) exactly, the warped scores are the f32 quotient logits / temperature bit for bit, and the draw
returns the fp64 inverse CDF's token at u = 0, at u = 1 - 2^-24 and at the midpoint of every CDF step wider than 1e-3.
tests/test_decode_select_fixtures_cpu.py proves that none of these cases hangs on rounding."""
import ctypes as C

import pytest
import torch

from tests import sample_ref as S

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")


def _lib():
    from klab_multimodalmodel_amd import _lib as L
    return L, L.load()


class _Rows:
    """the fixture's rows on the device in one layout -- aligned: ld = ld_warped = V; odd: ld = V + 3, ld_warped = V + 1, both from a
    base one element past an aligned address; the gap columns hold +60 (a read past V would be the maximum)"""

    def __init__(self, x, odd):
        self.R, self.V = x.shape
        self.dtype = x.dtype
        self.ld, self.ldw, self.off = (self.V + 3, self.V + 1, 1) if odd else (self.V, self.V, 0)
        xb = torch.full((self.off + self.R * self.ld + 8,), 60.0, dtype=x.dtype)
        xb[self.off:self.off + self.R * self.ld].view(self.R, self.ld)[:, :self.V] = x
        self.xb = xb.cuda()

    def run(self, t, k, p, u, row_div, want_warped):
        """rows = R * row_div draws (row r reads logits row r / row_div with u[r]); returns (tokens, warped or None, the warped
        buffer's gap columns and ends)"""
        L, lib = _lib()
        rows = self.R * row_div
        tok = torch.full((rows,), -1, dtype=torch.int64, device="cuda")
        u_d = u.float().cuda()
        wb = torch.full((self.off + rows * self.ldw + 8,), NAN, device="cuda") if want_warped else None
        a = L.SampleArgs()
        a.dtype, a.logits, a.ld, a.row_div, a.rows, a.V = (L.dtype_code(self.dtype), self.xb.data_ptr() + self.off * self.xb.element_size(), self.ld,
                                                           row_div, rows, self.V)
        a.temperature, a.top_k, a.top_p, a.seed, a.step = t, k, p, 0, 1
        a.u_in, a.tokens = u_d.data_ptr(), tok.data_ptr()
        a.warped, a.ld_warped = (wb.data_ptr() + self.off * 4, self.ldw) if want_warped else (None, 0)
        L.check(lib.klab_sample_rows(C.byref(a), L.stream_ptr()), "klab_sample_rows")
        torch.cuda.synchronize()
        if not want_warped:
            return tok.cpu(), None, None
        wb = wb.cpu()
        view = wb[self.off:self.off + rows * self.ldw].view(rows, self.ldw)
        return tok.cpu(), view[:, :self.V].clone(), torch.cat((wb[:self.off], view[:, self.V:].reshape(-1), wb[self.off + rows * self.ldw:]))


@pytest.mark.parametrize("dn", ["f32", "bf16"])
@pytest.mark.parametrize("V", S.SAMPLE_VOCABS)
def test_sample_rows_exact(V, dn):
    x = S.sample_fixture(V, dn)
    x32 = x.float()
    layouts = [_Rows(x.to(DT[dn]), False), _Rows(x.to(DT[dn]), True)]
    settings = S.sample_settings(V, dn, S.TEMPERATURES if V < 32768 else (1.0,))
    n_u = 16
    for n, (t, k, p, _plain) in enumerate(settings):
        want = S.kept_reference(x32, t, k, p)
        sc = S.scaled(x32, t)
        # the draws: up to n_u per logits row in one launch (row_div); the unused slots repeat the row's first
        pts = S.draw_points(x32, t, want)
        per_row = [[q for q in pts if q[0] == r] for r in range(8)]
        assert max(len(q) for q in per_row) <= n_u and min(len(q) for q in per_row) >= 1, (V, dn, t, k, p)
        u = torch.zeros(8, n_u, dtype=torch.float64)
        exp = torch.empty(8, n_u, dtype=torch.int64)
        for r, q in enumerate(per_row):
            q = q + [q[0]] * (n_u - len(q))
            u[r] = torch.tensor([z[1] for z in q], dtype=torch.float64)
            exp[r] = torch.tensor([z[2] for z in q])
        for dev in (layouts if V < 32768 else layouts[n % 2:n % 2 + 1]):  # the large vocabulary alternates the layouts
            what = (V, dn, t, k, p, dev.off)
            _, warped, gaps = dev.run(t, k, p, torch.zeros(8), 1, True)
            assert bool(torch.isnan(gaps).all()), what  # nothing written past V
            assert not torch.isnan(warped).any(), what
            got = ~torch.isinf(warped)
            assert torch.equal(got, want), (what, torch.nonzero(got != want)[:8])
            assert torch.equal(warped[want], sc[want]) and bool((warped[~want] == -float("inf")).all()), what
            tok, _, _ = dev.run(t, k, p, u.reshape(-1), n_u, False)  # (u is rounded to f32: the CPU test bounds what that moves)
            tok = tok.view(8, n_u)
            assert torch.equal(tok, exp), (what, torch.nonzero(tok != exp)[:8], tok, exp)
