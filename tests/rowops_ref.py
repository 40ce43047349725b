"""fp64 / f32 references, fixtures, bounds and the dropout hash for tests/test_norm_exact_gpu.py, tests/test_loss_act_exact_gpu.py
and tests/test_glue_exact_gpu.py (plain numpy / torch on the CPU; tests/test_rowops_fixtures_cpu.py proves what the GPU tests take
for granted about them).

Three kinds of statement are made about a row kernel:
  (a) its row statistic (rstd, mean) against fp64 under a first-order worst-case bound of the f32 summation (adds());
  (b) its outputs as the fixed f32 expression of ITS OWN statistic: every product in these expressions is either the only
      operation or exact, so that fusing a multiply into the following add changes nothing and torch.equal is a fair demand;
  (c) randn operands end to end against fp64, per element.
The backward fixtures choose rstd in {1, 1/2, 1/4}, x (or y - mean) in {0, +-1, +-2, +-4} and small integers elsewhere: the row
dot products are exact integers (or multiples of 1/4), x * k is an exact product, and the weight-gradient column sums are exact
in any order.

drop_mult is the one Python statement of the dropout mask keep(seed, tag, index) of csrc/common.h."""
import functools
import math

import numpy as np
import torch

from tests.exact_ref import U8, U24, gen, ints

M32 = np.uint64(0xFFFFFFFF)
GUARD = 256  # elements of guard band on either side of every output


# ---- the dropout hash ----------------------------------------------------------------------------------------------------------
def mix32(x):
    """the 32-bit finaliser of common.h on a uint64 array that holds 32-bit values"""
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def drop_hash(seed, tag, idx):
    """the 32-bit hash of element `idx` (any integer array, up to 64 bits) under (seed, tag)"""
    idx = np.asarray(idx).astype(np.uint64)
    key = mix32(np.uint64((int(seed) * 0x9E3779B1 + int(tag) * 0x7FEB352D + 0x165667B1) & 0xFFFFFFFF))
    lo, hi = idx & M32, idx >> np.uint64(32)
    h = mix32((lo * np.uint64(0x9E3779B1) + key) & M32)
    h2 = mix32(h ^ ((hi * np.uint64(0x85EBCA77) + np.uint64(0x27D4EB2F)) & M32))
    return np.where(hi != 0, h2, h)


def drop_mult(seed, tag, p, idx):
    """f32 multiplier of element idx: 0 where hash < trunc(p 2^32), else 1 / (1 - p) in f32 arithmetic"""
    pf = np.float32(p)
    thresh = min(int(float(pf) * 4294967296.0), 0xFFFFFFFF)
    scale = np.float32(1.0) / (np.float32(1.0) - pf)
    h = drop_hash(seed, tag, idx)
    return np.where(h < np.uint64(thresh), np.float32(0.0), scale).astype(np.float32)


def remap_rows(rows, grp=0, grp_stride=0, off=0):
    """the output row of every input row: (row / grp) * grp_stride + off + row % grp, the identity for grp <= 0"""
    r = torch.arange(rows, dtype=torch.int64)
    if grp <= 0:
        return r
    return (r // grp) * grp_stride + off + r % grp


def out_rows(rows, grp=0, grp_stride=0, off=0):
    """rows of the smallest buffer that holds every remapped row"""
    return int(remap_rows(rows, grp, grp_stride, off).max()) + 1


def mask(seed, tag, p, rowidx, width):
    """torch f32 [len(rowidx), width] of multipliers at element index rowidx * width + c"""
    idx = rowidx.numpy().astype(np.uint64)[:, None] * np.uint64(width) + np.arange(width, dtype=np.uint64)[None, :]
    return torch.from_numpy(drop_mult(seed, tag, p, idx))


# ---- bounds --------------------------------------------------------------------------------------------------------------------
def adds(n, lanes=64):
    """longest chain of f32 additions when `lanes` lanes sum n values four at a time and fold by shuffles"""
    return 4 * math.ceil(n / (4 * lanes)) + int(math.log2(lanes)) + 4


def ln_lanes(C):
    """lanes per row of layernorm_fwd_kernel"""
    return 16 if C <= 64 else 32 if C <= 128 else 64


def first_bad(name, got, want, extra=""):
    """message naming the output and its first wrong element (got, want: CPU tensors of one shape)"""
    bad = ~((got == want) | (torch.isnan(got.double()) & torch.isnan(want.double()))) if got.is_floating_point() else got != want
    if not bool(bad.any()):
        return None
    i = bad.flatten().nonzero()[0].item()
    pos = np.unravel_index(i, tuple(got.shape)) if got.dim() else ()
    return (f"{name}{extra}: {int(bad.sum())} of {bad.numel()} elements wrong, first at {tuple(int(v) for v in pos)}: "
            f"got {got.flatten()[i].item()!r}, want {want.flatten()[i].item()!r}")


def assert_equal(name, got, want, extra=""):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{name}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    msg = first_bad(name, got, want, extra)
    assert msg is None, msg


def assert_within(name, got, ref, bound, extra=""):
    """|got - ref| <= bound element-wise (fp64); prints the worst err / bound, names the first offender"""
    got, ref, bound = got.cpu().double(), ref.double(), torch.as_tensor(bound).double()
    bound = bound.expand_as(ref) if bound.dim() else bound * torch.ones_like(ref)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isnan(got) | torch.isnan(ratio), torch.full_like(err, math.inf), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{name}{extra}: max |err| {float(err[~torch.isnan(err)].max()) if err.numel() else 0.0:.3e}, worst err / bound {worst:.3f}")
    if worst > 1.0:
        i = (ratio > 1.0).flatten().nonzero()[0].item()
        pos = np.unravel_index(i, tuple(ref.shape)) if ref.dim() else ()
        raise AssertionError(f"{name}{extra}: {int((ratio > 1.0).sum())} of {ratio.numel()} elements out of bound (worst ratio {worst:.3f}), first at "
                             f"{tuple(int(v) for v in pos)}: got {got.flatten()[i].item()!r}, want {ref.flatten()[i].item()!r}, "
                             f"bound {bound.flatten()[i].item():.3e}")
    return worst


class Guarded:
    """an output tensor between two guard bands of GUARD elements.  Overwritten outputs start as NaN (0xA5 for bytes), accumulated
    ones from `init`; check() demands the bands untouched."""
    SENT = {torch.uint8: 0x5A, torch.int32: -12345}

    def __init__(self, shape, dtype, device="cuda", init=None):
        n = int(np.prod(shape))
        self.sent = self.SENT.get(dtype, -77.0)
        self.buf = torch.full((n + 2 * GUARD,), self.sent, dtype=dtype, device=device)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if init is not None:
            self.t.copy_(init)
        elif dtype.is_floating_point:
            self.t.fill_(float("nan"))
        else:
            self.t.fill_(0xA5 if dtype == torch.uint8 else -1)

    def check(self, name):
        b = self.buf.cpu()
        lo, hi = b[:GUARD], b[-GUARD:]
        assert bool((lo == self.sent).all()), f"{name}: guard band in front overwritten at {(lo != self.sent).nonzero().flatten()[:4].tolist()}"
        assert bool((hi == self.sent).all()), f"{name}: guard band behind overwritten at {(hi != self.sent).nonzero().flatten()[:4].tolist()}"
        return self.t.cpu()


def scatter_rows(orow, want, total_rows, fill=float("nan")):
    """expected image of a remapped output: `want` rows at orow, `fill` (what the buffer started with) everywhere else"""
    full = torch.full((total_rows, want.shape[1]), fill, dtype=want.dtype)
    full[orow] = want
    return full


# ---- fp8 rows ------------------------------------------------------------------------------------------------------------------
def q8_expected(y_bf16):
    """(bytes uint8, scales f32) of a bf16 row image: scale = f32(amax * f32(1 / 448)), 1 for an all-zero row; bytes =
    clamp(y * f32(1 / scale), +-448) rounded to nearest-even e4m3"""
    y = y_bf16.float()
    amax = y.abs().amax(dim=-1, keepdim=True)
    sc = torch.where(amax > 0, amax * torch.tensor(1.0 / 448.0, dtype=torch.float32), torch.ones_like(amax))
    inv = torch.ones_like(sc) / sc
    q = (y * inv).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, sc[..., 0]


def unsigned_zero(b):
    """e4m3 bytes with -0 (0x80) folded onto +0: the sign of a zero is nobody's contract"""
    return torch.where(b == 0x80, torch.zeros_like(b), b)


# ---- RMS-norm ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rms_randn(rows, d, seed=0):
    """x = 2 randn, w = 1 + 0.1 randn (f32), the fp64 rstd and normalised product.  Cached: callers must not write into it."""
    g = gen(7000 + seed)
    x = (2.0 * torch.randn(rows, d, generator=g)).float()
    w = (1.0 + 0.1 * torch.randn(d, generator=g)).float()
    r = (x.double().pow(2).mean(-1) + 1e-6).rsqrt()
    return dict(x=x, w=w, r=r, y=x.double() * r[:, None] * w.double())


def rms_fwd_from_stat(x, w, r_k, mult=None):
    """y as the kernel must compute it from the rstd it wrote: w * (x * r) [* mult], every step one f32 rounding"""
    o = w[None, :] * (x * r_k[:, None])
    return o if mult is None else o * mult


def pick(g, values, *shape):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=g)]


@functools.lru_cache(maxsize=None)
def rms_bwd_fixture(rows, d, seed=0):
    """the exact fixture of the RMS-norm backward (fp64 tensors holding f32-exact values)"""
    g = gen(7100 + seed + 13 * rows + d)
    return dict(rstd=pick(g, (1.0, 0.5, 0.25), rows), x=pick(g, (0.0, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0), rows, d), w=ints(g, -3, 3, d),
                dy=ints(g, -3, 3, rows, d), dres=ints(g, -8, 8, rows, d), dw0=ints(g, 1, 5, d))


def rms_bwd_exact(fx, my=None, mp=None, use_dres=True):
    """f32 evaluation in the kernel's order (rms_bwd_fixture operands; my / mp the f32 multipliers of dy and of dxt, or None).
    Returns dx (f32), dxt32 (f32: dx times mp, to be rounded by the caller), dwsum (fp64 column sums of de x r) and the pieces the
    CPU test inspects."""
    x, w, dy, r = fx["x"], fx["w"], fx["dy"], fx["rstd"]
    de = dy if my is None else dy * my.double()
    dot = (de * w[None, :] * x).sum(-1)  # exact integer
    d = x.shape[1]
    k = (dot * r ** 3).float() / torch.tensor(float(d), dtype=torch.float32)  # one rounding: the division
    a = (r[:, None] * w[None, :] * de).float()  # exact
    b = x.float() * k[:, None]                   # exact: x is 0 or a power of two
    t = a - b
    dx = t + fx["dres"].float() if use_dres else t
    dxt32 = dx if mp is None else dx * mp
    return dict(dx=dx, dxt32=dxt32, dwsum=(de * x * r[:, None]).sum(0), dot=dot, k=k, a=a, b=b, de=de)


def rms_bwd_fma(fx, my=None, mp=None, use_dres=True):
    """the same with x * k folded into the subtraction (fp64 holds the exact product of two f32, the result is rounded once)"""
    e = rms_bwd_exact(fx, my, mp, use_dres)
    t = (e["a"].double() - fx["x"] * e["k"].double()[:, None]).float()
    return t + fx["dres"].float() if use_dres else t


def rms_bwd_reference(x, w, dy, r, dres, my=None):
    """fp64 backward of randn operands from the rstd handed to the kernel, with the companions of the per-element bound"""
    x, w, dy, r = x.double(), w.double(), dy.double(), r.double()
    de = dy if my is None else dy * my.double()
    d = x.shape[1]
    k = (de * w[None] * x).sum(-1) * r ** 3 / d
    a, b = r[:, None] * w[None] * de, x * k[:, None]
    dx = a - b + (dres.double() if dres is not None else 0.0)
    n = adds(d)
    bound = U24 * ((n + 8) * x.abs() * (r ** 3 / d)[:, None] * (de * w[None] * x).abs().sum(-1, keepdim=True) + 6 * (a.abs() + b.abs())
                   + (2 * dres.double().abs() if dres is not None else 0.0))
    term = de * x * r[:, None]
    return dict(dx=dx, bound=bound, dw=term.sum(0), dw_bound=2 * x.shape[0] * U24 * term.abs().sum(0))


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------
GAMMAS = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)


@functools.lru_cache(maxsize=None)
def ln_randn(rows, C, seed=0):
    """y = 2 randn rounded to bf16 (both input dtypes are fed the same values), gamma from GAMMAS, beta and shortcut randn; a second
    gamma2 = 1 + 0.1 randn for the end-to-end bound; integer rows yi in [-8, 8]; fp64 mean and rstd of y and of yi"""
    g = gen(7200 + seed)
    y = (2.0 * torch.randn(rows, C, generator=g)).to(torch.bfloat16).float()
    yi = ints(g, -8, 8, rows, C).float()
    out = dict(y=y, yi=yi, gamma=pick(g, GAMMAS, C).float(), gamma2=(1.0 + 0.1 * torch.randn(C, generator=g)).float(),
               beta=torch.randn(C, generator=g).float(), shortcut=torch.randn(rows, C, generator=g).float())
    for k, v in (("", y), ("i", yi)):
        mu = v.double().mean(-1)
        out["mu" + k] = mu
        out["r" + k] = ((v.double() - mu[:, None]).pow(2).mean(-1) + 1e-5).rsqrt()
    return out


def ln_fwd_from_stat(y, mu_k, r_k, gamma, beta, shortcut=None, mult=None):
    """out = f32(f32(f32(f32(y - mu) r) gamma + beta) + shortcut) [* mult]: gamma is 0 or a power of two, so the product that a
    fused multiply-add would keep unrounded is exact anyway"""
    o = ((y - mu_k[:, None]) * r_k[:, None]) * gamma[None, :] + beta[None, :]
    if shortcut is not None:
        o = o + shortcut
    return o if mult is None else o * mult


def ln_fwd_reference(y, gamma, beta, shortcut, C):
    """fp64 forward and the bound of (c).  The output is a SUM (xhat gamma + beta + shortcut) of a DIFFERENCE (y - mean), so the
    error is relative to the sum of the absolute terms, not to the result: (adds + 12) 2^-24 (|xhat gamma| + |beta| + |shortcut|),
    plus what the error of the mean (adds 2^-24 sum|y| / C + 2^-24 |mu|) does through r |gamma|"""
    y, gamma, beta = y.double(), gamma.double(), beta.double()
    mu = y.mean(-1, keepdim=True)
    r = ((y - mu).pow(2).mean(-1, keepdim=True) + 1e-5).rsqrt()
    xg = (y - mu) * r * gamma[None]
    sc = shortcut.double() if shortcut is not None else torch.zeros_like(y)
    ref = xg + beta[None] + sc
    n = adds(C, ln_lanes(C))
    dmu = n * U24 * y.abs().sum(-1, keepdim=True) / C + U24 * mu.abs() + U24 * y.abs()  # (the last term: the rounding of y - mu)
    bound = (n + 12) * U24 * (xg.abs() + beta.abs()[None] + sc.abs()) + 2 * r * gamma.abs()[None] * dmu
    return ref, bound


@functools.lru_cache(maxsize=None)
def ln_bwd_fixture(rows, C, seed=0):
    g = gen(7300 + seed + 13 * rows + C)
    mean = pick(g, (0.0, 1.0), rows)
    return dict(mean=mean, rstd=pick(g, (1.0, 0.5, 0.25), rows), y=mean[:, None] + pick(g, (0.0, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0), rows, C),
                gamma=ints(g, -3, 3, C), dout=ints(g, -3, 3, rows, C), dgamma0=ints(g, 1, 5, C), dbeta0=ints(g, 1, 5, C),
                dprev0=ints(g, 1, 5, C))


def ln_bwd_exact(fx, m=None):
    """dy = r f32(f32(gamma de - s1) - xhat s2) with s1, s2 exact sums divided once; dgamma, dbeta exact column sums (fp64)"""
    y, mu, r, g = fx["y"], fx["mean"], fx["rstd"], fx["gamma"]
    C = y.shape[1]
    de = fx["dout"] if m is None else fx["dout"] * m.double()
    xh = (y - mu[:, None]) * r[:, None]              # exact
    Cf = torch.tensor(float(C), dtype=torch.float32)
    s1n, s2n = (g[None] * de).sum(-1), (g[None] * de * xh).sum(-1)  # exact
    s1, s2 = s1n.float() / Cf, s2n.float() / Cf
    t1 = (g[None] * de).float() - s1[:, None]
    p2 = xh.float() * s2[:, None]                    # exact: xhat is 0 or a power of two
    dy = r.float()[:, None] * (t1 - p2)
    return dict(dy=dy, dgamma=(de * xh).sum(0), dbeta=de.sum(0), s1n=s1n, s2n=s2n, s2=s2, xh=xh, t1=t1, de=de)


def ln_bwd_fma(fx, m=None):
    e = ln_bwd_exact(fx, m)
    return fx["rstd"].float()[:, None] * (e["t1"].double() - e["xh"] * e["s2"].double()[:, None]).float()


def ln_bwd_reference(y, gamma, mean, rstd, dout, m=None):
    """fp64 LayerNorm backward from the statistics handed to the kernel, and the per-element bound of dy"""
    y, g, mu, r, do = y.double(), gamma.double(), mean.double(), rstd.double(), dout.double()
    C = y.shape[1]
    de = do if m is None else do * m.double()
    xh = (y - mu[:, None]) * r[:, None]
    gd = g[None] * de
    s1, s2 = gd.sum(-1, keepdim=True) / C, (gd * xh).sum(-1, keepdim=True) / C
    dy = r[:, None] * (gd - s1 - xh * s2)
    n = adds(C)
    bound = U24 * r[:, None] * ((n + 8) / C * (gd.abs().sum(-1, keepdim=True) + xh.abs() * (gd * xh).abs().sum(-1, keepdim=True))
                                + 8 * (gd.abs() + s1.abs() + (xh * s2).abs()))
    rows = y.shape[0]
    return dict(dy=dy, bound=bound, dgamma=(de * xh).sum(0), dgamma_bound=2 * rows * U24 * (de * xh).abs().sum(0), dbeta=de.sum(0),
                dbeta_bound=2 * rows * U24 * de.abs().sum(0))


# ---- the shapes ----------------------------------------------------------------------------------------------------------------
RMS_FWD = [(r, d) for d in (4, 132, 256, 260, 1028) for r in (1, 5)] + [(8197, 132)]
RMS_Q8 = [(r, d) for d in (8, 132, 256, 260, 512, 516, 1024) for r in (5, 77)]
RMS_BWD = [(r, d) for d in (12, 132, 256, 260, 512, 516, 1024) for r in (1, 17, 8200)]
RMS_BWD_SPLIT = [(17, 132, False), (300, 1028, True)]  # (rows, d, dw given)
LN_FWD = ([(r, C) for C in (4, 16, 64) for r in (1, 3, 5)] + [(32771, 16)] + [(r, C) for C in (68, 96, 128) for r in (1, 3)] + [(16387, 68)]
          + [(5, C) for C in (132, 256, 260, 1536)] + [(8197, 132)])
LN_Q8 = [(7, C) for C in (16, 96, 132, 1024)]
LN_BWD = [(r, C) for C in (16, 132, 256, 260, 516, 1024) for r in (1, 17, 8200)]
LN_BWD_SUBSETS = [(17, 132), (300, 64)]
LN_BWD_SPLIT = [(37, 1028, "f32"), (37, 1032, "bf16")]
LN_DPREV_EXACT = (300, 64)  # dprev_bias is an exact sum here (proved by the CPU test)
REMAP = dict(grp=3, grp_stride=5, off=1)


# ---- cross-entropy -------------------------------------------------------------------------------------------------------------
CE_V = {"bf16": (8, 2056, 16384, 16392, 32768, 32776, 40000), "f32": (4, 1028, 4104)}
CE_PAD = 16      # ld = V + CE_PAD, the columns behind V hold CE_SENT and must survive
CE_SENT = 777.0


def expf_rel(z):
    """relative error allowed to __expf(z): 2^-24 (2 |z| + 4)"""
    return U24 * (2.0 * z.abs() + 4.0)


@functools.lru_cache(maxsize=None)
def ce_case(rows, V, dt):
    """logits 3 randn with one -200 and one +20 per row, as the dtype stores them (fp64 holds them); labels at column 0, V - 1,
    inside the last 16-byte vector, -100, the middle and at random; the fp64 reference and the per-element bounds"""
    g = gen(7600 + V + rows)
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    x = 3.0 * torch.randn(rows, V, generator=g)
    cols = torch.stack([torch.randperm(V, generator=g)[:2] for _ in range(rows)])
    x[torch.arange(rows), cols[:, 0]] = -200.0
    x[torch.arange(rows), cols[:, 1]] = 20.0
    stored = x.to(dtype)
    x = stored.double()
    lab = torch.randint(0, V, (rows,), generator=g)
    fixed = torch.tensor([0, V - 1, max(V - 3, 0), -100, V // 2])
    for i in range(0, rows - 4, 87):
        lab[i:i + 5] = fixed
    valid = lab != -100
    n = int(valid.sum())
    inv_n = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    mx = x.amax(-1, keepdim=True)
    lse = torch.logsumexp(x, -1, keepdim=True)
    p = (x - lse).exp()
    a = 8 * math.ceil(V / 2048) + 12
    dlse = (p * expf_rel(x - mx)).sum(-1, keepdim=True) + U24 * (a + 2 * lse.abs() + 16)
    safe = lab.clamp_min(0)
    loss_row = torch.where(valid, lse[:, 0] - x[torch.arange(rows), safe], torch.zeros(rows, dtype=torch.float64))
    row_bound = torch.where(valid, dlse[:, 0] + U24 * loss_row.abs(), torch.zeros(rows, dtype=torch.float64))
    delta = torch.zeros_like(x)
    delta[torch.arange(rows)[valid], lab[valid]] = 1.0
    inv = float(inv_n)
    grad = torch.where(valid[:, None], inv * (p - delta), torch.zeros_like(x))
    gbound = inv * (p * (expf_rel(x - lse) + dlse) + 2 * U24 * (p - delta).abs()) + 2.0 ** -120
    if dt == "bf16":
        gbound = gbound + U8 * grad.abs()
    gbound = torch.where(valid[:, None], gbound, torch.zeros_like(x))
    loss = inv * loss_row.sum()
    loss_bound = inv * (row_bound.sum() + 2 * (rows / 256 + 12) * U24 * loss_row.abs().sum())
    return dict(stored=stored, labels=lab, valid=valid, inv_n=inv_n, loss_row=loss_row, row_bound=row_bound, grad=grad, gbound=gbound, loss=loss,
                loss_bound=loss_bound, dtype=dtype)


# ---- GELU ----------------------------------------------------------------------------------------------------------------------
C0, C1 = math.sqrt(2.0 / math.pi), 0.044715


def all_finite_bf16():
    """the 65280 finite bf16 bit patterns as a [16, 4080] bf16 matrix"""
    bits = np.arange(1 << 16, dtype=np.uint16)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    assert bits.size == 65280
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16).view(16, 4080)


def gelu_erf64(x):
    """0.5 x (1 + erf(x / sqrt 2)) in fp64, through erfc on the negative side (no cancellation)"""
    x = x.double()
    return torch.where(x < 0, 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0)), 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0))))


def pdf64(x):
    x = x.double()
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_new64(x):
    """(value, derivative) of 0.5 x (1 + tanh(c0 (x + c1 x^3))) = x sigmoid(2 u) in fp64, the derivative by autograd"""
    x = x.double().clone().requires_grad_(True)
    y = x * torch.sigmoid(2.0 * C0 * x * (1.0 + C1 * x * x))
    (dy,) = torch.autograd.grad(y.sum(), x)
    return y.detach(), dy


def gelu_f32_bound(x, ref):
    """f32 forms (libm erff / tanhf): 8 2^-24 (|ref| + |x| pdf(x)) as the issue states it, and the term it lacks: 1 + erf (1 + tanh)
    is a sum with an absolute error of about 2 2^-24 whatever its size, and it is multiplied by x / 2 -- on the negative side, where
    the sum cancels, that is all there is: + 2 2^-24 |x|.  Returns (stated, used)."""
    x = x.double()
    stated = 8 * U24 * (ref.abs() + x.abs() * pdf64(x))
    return stated, stated + 2 * U24 * x.abs()


def gelu_new_grad_f32_bound(x, ref):
    """derivative hp + 0.5 x (1 - t^2) k(x), k = c0 (1 + 3 c1 x^2): 8 roundings on the result, and the two sums 1 + t and 1 - t^2
    with absolute errors of 2 and 4 units: 2^-24 (8 |ref| + 4 (1 + |x| k(x)))"""
    x = x.double()
    return U24 * (8 * ref.abs() + 4 * (1.0 + x.abs() * C0 * (1.0 + 3 * C1 * x * x)))


GELU_NEW_C = 1.0  # factor c of the bf16 gelu_new bound 2^-8 |ref| + c 1e-7 (|a| + 1) |b|


def gelu_new_bf16_bound(a, scale, ref, c=GELU_NEW_C):
    """scale: what the activation (or its derivative) is multiplied by (|b|, |dh mult|, ...)"""
    return U8 * ref.abs() + c * 1e-7 * (a.double().abs() + 1.0) * scale


def gelu_new_grad_bf16_bound(a, scale, ref, c=GELU_NEW_C):
    """the derivative hp + 0.5 x (1 - t^2) k(x), k = c0 (1 + 3 c1 x^2): the ~1e-7 of t enters through 1 - t^2 (2 |t| 1e-7) times
    0.5 |x| k(x), i.e. the expression of the value times the polynomial 1 + 3 c1 x^2 -- capped at |x| = 6, beyond which t is +-1
    exactly and 1 - t^2 is 0"""
    a = a.double()
    return U8 * ref.abs() + c * 1e-7 * (a.abs() + 1.0) * (1.0 + 3 * C1 * a.pow(2).clamp_max(36.0)) * scale
