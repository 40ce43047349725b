"""The harness tests/test_attn_exact_gpu.py and tests/test_attn_fused_exact_gpu.py share: every output of an attention kernel sits in
a sentinel-filled buffer with a leading dimension larger than needed and guard rows (matrices) or guard elements (flat arrays), and
is fetched through a check that nothing outside the written region changed; comparisons name the output and the first wrong
(b, h, row, col)."""
import torch

from tests import exact_ref as R

GUARD = 16      # elements before and after the flat f32 / bf16 outputs (lse, dbias, the dS slab)
REL = 2.0 ** -20
PAD_VALUE = 7.0


def rows(x):
    """[B, H, L, dk] -> [B * L, H * dk]: head h at column h * dk"""
    return R.unheads(x)


def unrows(x, L, H):
    return R.heads(x, L, H)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def sentinel(shape, dtype):
    buf = torch.empty(shape, dtype=dtype)
    if dtype == torch.float32:
        buf.view(torch.int32).fill_(0x5A5B5C5D)
    else:
        buf.view(torch.int16).fill_(0x5A5B)
    return buf


def fused_input(parts, dtype, pad=8):
    """column blocks side by side in one [rows, sum of widths + pad] buffer -> (device buffer, ld, views at each block's first column)"""
    mats = [rows(p) if p.dim() == 4 else p for p in parts]
    w = mats[0].shape[1]
    buf = torch.full((mats[0].shape[0], w * len(mats) + pad), PAD_VALUE, dtype=dtype)
    for i, m in enumerate(mats):
        buf[:, i * w:(i + 1) * w] = m.to(dtype)
    d = buf.cuda()
    return d, buf.shape[1], [d[:, i * w:] for i in range(len(mats))]


class MatOut:
    """`nblk` output matrices [n, H dk] side by side in a sentinel-filled [n + 2, nblk H dk + 8] buffer, written from row 1 on"""

    def __init__(self, n, width, nblk, dtype, H):
        self.n, self.w, self.nblk, self.H = n, width, nblk, H
        self.ld = width * nblk + 8
        self.before = sentinel((n + 2, self.ld), dtype)
        self.buf = self.before.cuda()
        self.views = [self.buf[1:, i * width:] for i in range(nblk)]

    def fetch_rows(self):
        """-> the blocks as [n, width] matrices; asserts that nothing outside them changed"""
        after = self.buf.cpu()
        got = [after[1:1 + self.n, i * self.w:(i + 1) * self.w].clone() for i in range(self.nblk)]
        after[1:1 + self.n, :self.w * self.nblk] = self.before[1:1 + self.n, :self.w * self.nblk]
        touched = bits(after) != bits(self.before)
        assert not bool(touched.any()), f"wrote outside the output matrix at (buffer row, column) {touched.nonzero()[:8].tolist()}"
        return got

    def fetch(self, L):
        """-> the blocks as [B, H, L, dk]; asserts that nothing outside them changed"""
        return [unrows(m, L, self.H) for m in self.fetch_rows()]

    def assert_untouched(self, what):
        assert torch.equal(bits(self.buf.cpu()), bits(self.before)), f"{what}: the output buffer was written"


class FlatOut:
    """a flat output of n elements between two guards of sentinel; fill: what the n elements start from (None: sentinel too)"""

    def __init__(self, n, dtype, fill=None):
        self.n = n
        self.before = sentinel((n + 2 * GUARD,), dtype)
        if fill is not None:
            self.before[GUARD:GUARD + n] = fill
        self.buf = self.before.cuda()
        self.view = self.buf[GUARD:GUARD + n]

    def fetch(self):
        after = self.buf.cpu()
        got = after[GUARD:GUARD + self.n].clone()
        assert torch.equal(bits(after[:GUARD]), bits(self.before[:GUARD])) and torch.equal(bits(after[GUARD + self.n:]), bits(self.before[GUARD + self.n:])), \
            "wrote into the guard of a flat output"
        return got

    def assert_untouched(self, what):
        assert torch.equal(bits(self.buf.cpu()), bits(self.before)), f"{what}: the output buffer was written"


def first_bad(bad):
    return tuple(int(v) for v in bad.nonzero()[0])


def assert_bf16_equal(got, ref, what):
    want = R.to_bf16_via_f32(ref)
    bad = got != want
    if bool(bad.any()):
        i = first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong, first at (b, h, row, col) = {i}: got {float(got[i])}, "
                             f"want {float(want[i])}")
    assert torch.equal(got, want)


def assert_f32_close(got, ref, what, mag=None):
    """|got - ref| <= 2^-20 mag (mag = |ref| unless the output is a sum: then the sum of its terms' magnitudes), 0 where mag is 0"""
    mag = ref.abs() if mag is None else mag
    err = (got.double() - ref).abs()
    bad = ~(err <= REL * mag)
    if bool(bad.any()):
        i = first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements off, first at {i}: got {float(got[i])!r}, want {float(ref[i])!r}, "
                             f"allowed {REL * float(mag[i]):.3e}")


def ratio(got, ref, bound, what):
    """worst err / bound of one output (printed), and the message that names the element"""
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    i = first_bad(r == r.max())
    print(f"  {what}: max err / bound {float(r.max()):.3e} at {i}")
    return float(r.max()), f"{what}: worst element {i}: got {float(got[i])}, want {float(ref[i])}, bound {float(bound[i]):.3e}"
