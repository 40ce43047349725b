"""Fixtures, fp64 references and bounds for tests/test_frozen_tower_exact_gpu.py: the four Linear (+ GELU + Linear) + LayerNorm
(+ residual) kernels of the frozen Swin tower (csrc/swin_mlp.hip, csrc/swin_lin_ln.hip, csrc/swin_embed.hip).  Plain numpy /
torch on the CPU; tests/test_frozen_tower_fixtures_cpu.py proves what the GPU tests take for granted about them.

The kernels write no row statistic, so the statistic is read out of the output.

Level 1, integer operands.  x (pixels), weights and biases are small integers, every product sum is an integer below 2^24 and
therefore the same f32 number in any order.  fc1 of `mlp` has weights and bias in 8 Z: every pre-activation u is a multiple of 8,
where gelu_poly(u) is max(u, 0) bit for bit (gelu_poly_np restates common.h; the CPU test proves the equality), and the hidden
row h = relu(u) <= 2048 is held by bf16.  The last Linear's rows c and c + C / 2 are negatives of each other (weights and bias),
then one integer mu is added to every bias: the pre-norm row y has the mean mu exactly and d = y - mu is an integer
(|y| <= 256 where the kernel rounds y to bf16, so that the rounding changes nothing).  Four channels q_j of the first half
listen to one input column k_j alone with bias 1 (+ mu), and row r has a zero in column k_(r mod 4) (`mlp`: a hidden unit that
listens to one x column, which is <= 0 in that row): d[r, q_(r mod 4)] = 1.  With gamma = 1, beta = 0 there and a zero in the
shortcut of that row, out[r, p(r)] = f32(f32(f32(1 rho) 1) + 0) + 0 IS the kernel's rstd.  It is compared with fp64 under
(chain + 8) 2^-24 rstd, and every other element with f32(f32(f32(f32(d rho) gamma) + beta) + shortcut) of that very rho:
gamma is 0 or a power of two, so a fused multiply-add changes nothing (expected_out(fma=True)).  In the other rows the probe
channels carry d != 1 and a shortcut like any channel.

Fixtures are built once at the largest row count of a shape family; a smaller M takes the first M rows, so what the CPU test
proves of the master (coverage of every hidden unit, input column and operand element) holds for the weights of every case.

Level 2, randn operands: fp64 on the operands as stored, nothing rounded in between, and a per-element bound with factor 1:
delta_y per kernel (dy_*), pushed through the norm by norm_push (first order + stated remainder), plus the f32 LayerNorm terms
of rowops_ref.ln_fwd_reference with the kernel's own chain."""
import functools

import numpy as np
import torch

from tests.exact_ref import gen, ints
from tests.rowops_ref import GAMMAS, U8, U24, gelu_erf64, pick

EPS = float(np.float32(1e-5))  # the kernels take eps as a float
NPROBE = 4
GELU_SLOPE, GELU_POLY_ERR = 1.13, 1.2e-4  # max |gelu'| (1.1290 at |u| = 1.41) and the documented error of gelu_poly (common.h)


def chain(kernel, C):
    """longest f32 addition chain of the kernel's variance sum: C / 4 in-lane + two shuffles (+ three for the four waves of
    linear_ln, which meet through LDS)"""
    return C // 4 + 2 + (3 if kernel == "linear_ln" else 0)


# ---- gelu_poly of common.h in numpy f32 ----------------------------------------------------------------------------------------
GELU_Q = (7.318504830e-11, -7.769299870e-09, 3.614930506e-07, -9.785327165e-06, 1.732400560e-04, -2.146258019e-03, 1.943818480e-02,
          -1.324543953e-01, 7.977233529e-01)


def gelu_poly_np(x, fma):
    """gelu_poly on a float32 array; fma: every a * b + c rounded once (fp64 holds the product of two f32 exactly), else twice"""
    f = np.float32
    x = np.asarray(x, dtype=f)

    def mad(a, b, c):
        if fma:
            return (a.astype(np.float64) * b.astype(np.float64) + np.asarray(c, dtype=np.float64)).astype(f)
        return ((a * b).astype(f) + np.asarray(c, dtype=f)).astype(f)

    s = np.minimum((x * x).astype(f), f(20.48))
    q = np.full_like(x, f(GELU_Q[0]))
    for c in GELU_Q[1:]:
        q = mad(q, s, f(c))
    e = np.maximum(np.minimum((x * q).astype(f), f(1.0)), f(-1.0))
    hx = (x * f(0.5)).astype(f)
    return mad(hx, e, hx)


# ---- Level 1: integer fixtures -------------------------------------------------------------------------------------------------
def probe_channels(C):
    """four channels of the first half: different 16-channel tiles, different lane groups (c / 4 mod 4) and offsets in a lane"""
    return [1, C // 4 + 6, C // 2 - 5, C // 4 + 3]


def last_linear(g, K, C, mu, probe_in, lo, hi, density):
    """W [C, K], bias [C] of the Linear in front of the norm: rows c and c + C / 2 negatives of each other, + mu on the bias;
    channel probe_channels(C)[j] listens to input column probe_in[j] alone, with bias 1"""
    top = ints(g, lo, hi, C // 2, K) * (torch.rand(C // 2, K, generator=g) < density)
    b0 = ints(g, -4, 4, C // 2)
    for j, q in enumerate(probe_channels(C)):
        top[q] = 0.0
        top[q, probe_in[j]] = 1.0 if j % 2 == 0 else -1.0
        b0[q] = 1.0
    return torch.cat([top, -top]), torch.cat([b0, -b0]) + mu


def norm_operands(g, M, C, shortcut=True):
    """gamma from GAMMAS (1 at the probes), integer beta (0 at the probes), integer shortcut with a zero at (r, p(r))"""
    q = torch.tensor(probe_channels(C))
    probe = q[torch.arange(M) % NPROBE]
    gamma, beta = pick(g, GAMMAS, C), ints(g, -4, 4, C)
    gamma[q], beta[q] = 1.0, 0.0
    sc = ints(g, -8, 8, M, C)
    sc[sc == 0] = 3.0  # the only zeros are the probes'
    sc[torch.arange(M), probe] = 0.0
    if not shortcut:
        sc.zero_()
    return dict(gamma=gamma, beta=beta, sc=sc, probe=probe)


def zero_probe_inputs(a, probe_in):
    """row r gets a zero in column probe_in[r mod 4]; every other entry of those columns is made non-zero"""
    M = a.shape[0]
    cols = torch.tensor(probe_in)
    sub = a[:, cols]
    sub[sub == 0] = 2.0
    a[:, cols] = sub
    a[torch.arange(M), cols[torch.arange(M) % NPROBE]] = 0.0
    return a


def finish(fx, a, W, b, mu, C):
    """the exact pre-norm row and its statistics (fp64 holds all of it)"""
    y = a @ W.T + b[None]
    d = y - mu
    var = d.pow(2).sum(-1) / C
    fx.update(y=y, d=d, var=var, rho=(var + EPS).rsqrt(), absacc=a.abs() @ W.abs().T + b.abs()[None], mu=mu, C=C)
    return fx


PROJ_M = MLP_M = (1, 33, 128, 129, 300)
LINLN_M = {128: (1, 31, 33, 100), 160: (1, 31, 33, 100), 480: (1, 31, 33, 100), 512: (63, 65, 130), 544: (63, 65, 130), 1024: (63, 65, 130)}
EMBED_SHAPES = ((3, 12), (1, 32), (5, 28), (1, 4))  # (B, HW)
EMBED_PITCH = (64, 72)
MUS = (0, 3)


@functools.lru_cache(maxsize=None)
def proj_fixture(C, mu, M=max(PROJ_M)):
    g = gen(9100 + C + mu)
    pin = [0, C // 4 + 5, C // 2 + 6, C - 1]
    x = zero_probe_inputs(ints(g, -3, 3, M, C), pin)
    W, b = last_linear(g, C, C, mu, pin, -3, 3, 1.0)
    fx = dict(kernel="proj", x=x, W=W, b=b, probe_in=pin, **norm_operands(g, M, C))
    return finish(fx, x, W, b, mu, C)


@functools.lru_cache(maxsize=None)
def linln_fixture(K, mu, M=None, C=256):
    M = M or max(LINLN_M[K])
    g = gen(9200 + K + mu)
    pin = [0, 37, K // 2 + 5, K - 1]
    x = zero_probe_inputs(ints(g, -2, 2, M, K), pin)
    W, b = last_linear(g, K, C, mu, pin, -1, 1, min(0.75, 192.0 / K))
    fx = dict(kernel="linear_ln", x=x, W=W, b=b, probe_in=pin, **norm_operands(g, M, C))
    return finish(fx, x, W, b, mu, C)


def patches_to_pixels(a, B, HW):
    """[B R R, 48] patch rows (k = 16 c + 4 dy + dx) -> [B, 3, HW, HW]"""
    R = HW // 4
    return a.view(B, R, R, 3, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, HW, HW).contiguous()


@functools.lru_cache(maxsize=None)
def embed_weights(C, mu):
    g = gen(9300 + C + mu)
    pin = [0, 17, 30, 47]
    W, b = last_linear(g, 48, C, mu, pin, -2, 2, 1.0)
    return W, b, pin, norm_operands(g, 1, C, shortcut=False)


@functools.lru_cache(maxsize=None)
def embed_fixture(B, HW, C, mu):
    W, b, pin, no = embed_weights(C, mu)
    M = B * (HW // 4) ** 2
    a = zero_probe_inputs(ints(gen(9350 + 100 * B + HW), -3, 3, M, 48), pin)
    q = torch.tensor(probe_channels(C))
    fx = dict(kernel="patch_embed", x=a, pix=patches_to_pixels(a, B, HW), W=W, b=b, probe_in=pin, gamma=no["gamma"], beta=no["beta"],
              sc=torch.zeros(M, C, dtype=torch.float64), probe=q[torch.arange(M) % NPROBE])
    return finish(fx, a, W, b, mu, C)


def mlp_probe_units(C):
    """(hidden units, the x column each listens to)"""
    HD = 4 * C
    return [2, HD // 4 + 17, HD // 2 + 41, HD - 1], [3, C // 4 + 1, C // 2 + 6, C - 1]


@functools.lru_cache(maxsize=None)
def mlp_fixture(C, mu, M=max(MLP_M)):
    g = gen(9400 + C + mu)
    HD = 4 * C
    units, xcols = mlp_probe_units(C)
    x = ints(g, -2, 2, M, C)
    sub = x[:, xcols]
    sub[torch.arange(M), torch.arange(M) % NPROBE] = -sub[torch.arange(M), torch.arange(M) % NPROBE].abs()  # relu -> 0 in row r
    x[:, xcols] = sub
    W1 = 8.0 * pick(g, (-1.0, 0.0, 0.0, 1.0), HD, C)
    b1 = 8.0 * ints(g, -1, 1, HD)
    for n, k in zip(units, xcols):
        W1[n] = 0.0
        W1[n, k] = 8.0
        b1[n] = 0.0
    u = x @ W1.T + b1[None]
    h = u.clamp_min(0.0).float().to(torch.bfloat16).double()  # one RNE of the exact u (the CPU test: it changes nothing)
    W2, b2 = last_linear(g, HD, C, mu, units, -1, 1, 0.5)
    fx = dict(kernel="mlp", x=x, W1=W1, b1=b1, u=u, h=h, W=W2, b=b2, probe_in=units, absu=x.abs() @ W1.abs().T + b1.abs()[None],
              **norm_operands(g, M, C))
    return finish(fx, h, W2, b2, mu, C)


ROW_KEYS = ("x", "u", "h", "sc", "probe", "y", "d", "var", "rho", "absacc", "absu")


def take_rows(fx, M):
    """the first M rows of a master fixture"""
    return {k: (v[:M] if k in ROW_KEYS else v) for k, v in fx.items()}


def expected_out(fx, rho_k, fma=False):
    """f32(f32(f32(f32(d rho) gamma) + beta) + shortcut) from the kernel's own rstd (f32 [M]); fma: the product with gamma kept
    unrounded into the addition of beta"""
    t = fx["d"].float() * rho_k[:, None]
    gamma, beta, sc = fx["gamma"].float(), fx["beta"].float(), fx["sc"].float()
    if fma:
        o = (t.double() * gamma.double()[None] + beta.double()[None]).float()
    else:
        o = t * gamma[None] + beta[None]
    return o + sc


def reference_out(fx, **moved):
    """fp64 output of the fixture's operands, any of which may be replaced (the bite check): no exactness is assumed"""
    o = {**fx, **moved}
    if fx["kernel"] == "mlp":
        a = (o["x"] @ o["W1"].T + o["b1"][None]).clamp_min(0.0)
    else:
        a = o["x"]
    y = a @ o["W"].T + o["b"][None]
    d = y - y.mean(-1, keepdim=True)
    return d * (d.pow(2).mean(-1, keepdim=True) + EPS).rsqrt() * o["gamma"][None] + o["beta"][None] + o["sc"]


def visible(fx, ref, moved_ref):
    """does the exact test see the move?  The test as it runs, on the fp64 output of the moved operands: the rstd read at the probe
    leaves (chain + 8) 2^-24 rstd (by a factor of two), or some element differs from the expression of THAT rstd by more than
    8 2^-24 of its absolute terms -- the three roundings of the expression account for 3 2^-24 at the most"""
    n = chain(fx["kernel"], fx["C"])
    rows = torch.arange(ref.shape[0])
    rho_m = moved_ref[rows, fx["probe"]]
    if bool(((rho_m - fx["rho"]).abs() > 2 * (n + 8) * U24 * fx["rho"]).any()):
        return True
    xg = fx["d"] * rho_m[:, None] * fx["gamma"][None]
    want = xg + fx["beta"][None] + fx["sc"]
    terms = xg.abs() + fx["beta"].abs()[None] + fx["sc"].abs()
    return bool(((moved_ref - want).abs() > 8 * U24 * (terms + 1.0)).any())


def lattice_step(name, v):
    """the neighbouring lattice value of every element of an operand"""
    if name in ("W1", "b1"):
        return v + 8.0
    if name == "gamma":
        table = sorted(GAMMAS)
        idx = torch.tensor([table.index(float(t)) for t in v])
        return torch.tensor(table, dtype=torch.float64)[(idx + 1) % len(table)]
    return v + 1.0


# ---- Level 2: randn operands, fp64, per-element bounds -------------------------------------------------------------------------
def gterm(K, absprod):
    """f32 GEMM term of exact_ref.gemm_bound: 2 (K + 2) 2^-24 (sum |a| |b| + |bias|)"""
    return 2.0 * (K + 2) * U24 * absprod


def norm_push(y, dy, C):
    """(xhat, r, bound on |xhat' - xhat|) for any y' with |y' - y| <= dy element-wise.
    With d = y - mean(y), v = mean(d^2) + eps, r = v^-1/2, xhat = d r and delta' = delta - mean(delta), |delta'_c| <= E_c = dy_c + mean(dy):
        v' = v (1 + t),  t = 2 r mean(xhat delta') + r^2 mean(delta'^2),  |t| <= T = 2 r mean(|xhat| E) + r^2 mean(E^2)
        xhat' - xhat = r [delta' (1 + t)^-1/2 + d ((1 + t)^-1/2 - 1)],   (1 + t)^-1/2 = 1 - t / 2 + R(t)
    first order  r delta'_c - xhat_c r mean(xhat delta):   r (dy_c + mean(dy) + |xhat_c| mean(|xhat| dy))
    remainder    r delta'_c ((1 + t)^-1/2 - 1) + xhat_c (R(t) - r^2 mean(delta'^2) / 2).  Both (1 + t)^-1/2 - 1 and R are largest in
                 magnitude at t = -T (T < 1/2 asserted):  A = (1 - T)^-1/2 - 1  and  R(-T) = A - T / 2:
                 r E_c A + |xhat_c| (A - T / 2 + r^2 mean(E^2) / 2)"""
    mu = y.mean(-1, keepdim=True)
    d = y - mu
    r = (d.pow(2).mean(-1, keepdim=True) + EPS).rsqrt()
    xh = d * r
    E = dy + dy.mean(-1, keepdim=True)
    T = 2 * r * (xh.abs() * E).mean(-1, keepdim=True) + r * r * E.pow(2).mean(-1, keepdim=True)
    assert float(T.max()) < 0.5, float(T.max())
    A = (1.0 - T).rsqrt() - 1.0
    first = r * (dy + dy.mean(-1, keepdim=True) + xh.abs() * (xh.abs() * dy).mean(-1, keepdim=True))
    rem = r * E * A + xh.abs() * (A - T / 2 + r * r * E.pow(2).mean(-1, keepdim=True) / 2)
    return xh, r, first + rem


def out_bound(kernel, y, dy, gamma, beta, sc, C):
    """(ref, bound of out, bound of outt): |gamma| times the pushed delta_y, the f32 LayerNorm terms of
    rowops_ref.ln_fwd_reference with this kernel's chain, and one bf16 rounding for outt"""
    xh, r, dxh = norm_push(y, dy, C)
    xg = xh * gamma[None]
    ref = xg + beta[None] + sc
    n = chain(kernel, C)
    dmu = n * U24 * y.abs().sum(-1, keepdim=True) / C + U24 * y.mean(-1, keepdim=True).abs() + U24 * y.abs()
    bound = gamma.abs()[None] * dxh + (n + 12) * U24 * (xg.abs() + beta.abs()[None] + sc.abs()) + 2 * r * gamma.abs()[None] * dmu
    return ref, bound, bound + U8 * ref.abs()


def dy_plain(K, absacc):
    """proj: y is the f32 accumulator"""
    return gterm(K, absacc)


def dy_bf16_store(K, y, absacc):
    """linear_ln, patch_embed: y = bf16(acc + bias), half an ulp of the kernel's own sum"""
    return U8 * y.abs() + gterm(K, absacc) * (1.0 + U8)


def dy_mlp(C, absu, h, W2, b2):
    du = gterm(C, absu)
    dh = GELU_SLOPE * du + GELU_POLY_ERR + U8 * h.abs()
    return dh @ W2.abs().T + gterm(4 * C, h.abs() @ W2.abs().T + b2.abs()[None]), dh


def _norm_randn(g, M, C, shortcut=True):
    gamma = pick(g, (0.5, -0.5, 1.0, -1.0), C)
    beta = pick(g, (0.5, -0.5, 1.0, -1.0), C)
    sc = torch.randn(M, C, generator=g).float().double() if shortcut else torch.zeros(M, C, dtype=torch.float64)
    return gamma, beta, sc


def _bf(t):
    return t.to(torch.bfloat16).double()


@functools.lru_cache(maxsize=None)
def proj_randn(C, M=max(PROJ_M)):
    g = gen(9500 + C)
    x, W, b = _bf(torch.randn(M, C, generator=g)), _bf(torch.randn(C, C, generator=g) / C ** 0.5), (0.1 * torch.randn(C, generator=g)).float().double()
    gamma, beta, sc = _norm_randn(g, M, C)
    y = x @ W.T + b[None]
    ref, bo, bt = out_bound("proj", y, dy_plain(C, x.abs() @ W.abs().T + b.abs()[None]), gamma, beta, sc, C)
    return dict(kernel="proj", x=x, W=W, b=b, gamma=gamma, beta=beta, sc=sc, y=y, ref=ref, bound=bo, bound_t=bt, C=C)


@functools.lru_cache(maxsize=None)
def linln_randn(K, M=None, C=256):
    M = M or max(LINLN_M[K])
    g = gen(9600 + K)
    x, W, b = _bf(torch.randn(M, K, generator=g)), _bf(torch.randn(C, K, generator=g) / K ** 0.5), (0.1 * torch.randn(C, generator=g)).float().double()
    gamma, beta, sc = _norm_randn(g, M, C)
    y = x @ W.T + b[None]
    dy = dy_bf16_store(K, y, x.abs() @ W.abs().T + b.abs()[None])
    ref, bo, bt = out_bound("linear_ln", y, dy, gamma, beta, sc, C)
    return dict(kernel="linear_ln", x=x, W=W, b=b, gamma=gamma, beta=beta, sc=sc, y=y, dy=dy, ref=ref, bound=bo, bound_t=bt, C=C)


@functools.lru_cache(maxsize=None)
def embed_randn(B, HW, C):
    g = gen(9700 + C)
    W, b = _bf(0.1 * torch.randn(C, 48, generator=g)), (0.1 * torch.randn(C, generator=g)).float().double()
    M = B * (HW // 4) ** 2
    gamma, beta, sc = _norm_randn(g, M, C, shortcut=False)
    pix32 = torch.randn(B, 3, HW, HW, generator=gen(9750 + 100 * B + HW))  # f32, as the kernel is handed them
    R = HW // 4
    a = pix32.bfloat16().double().view(B, 3, R, 4, R, 4).permute(0, 2, 4, 1, 3, 5).reshape(M, 48)
    y = a @ W.T + b[None]
    dy = dy_bf16_store(48, y, a.abs() @ W.abs().T + b.abs()[None])
    ref, bo, bt = out_bound("patch_embed", y, dy, gamma, beta, sc, C)
    return dict(kernel="patch_embed", pix=pix32, x=a, W=W, b=b, gamma=gamma, beta=beta, sc=sc, y=y, dy=dy, ref=ref, bound=bo, bound_t=bt, C=C)


MLP_ROW_SCALE = (1.0, 2.0, 1.0, 3.0, 1.0, 2.0, 1.0, 12.0)  # u ~ N(0, scale^2): dense over (-5, 5), |u| up to about 40 in every eighth row


@functools.lru_cache(maxsize=None)
def mlp_randn(C, M=max(MLP_M)):
    g = gen(9800 + C)
    scale = torch.tensor(MLP_ROW_SCALE, dtype=torch.float32)[torch.arange(M) % len(MLP_ROW_SCALE)]
    x = _bf(torch.randn(M, C, generator=g) * scale[:, None])
    W1, W2 = _bf(torch.randn(4 * C, C, generator=g) / C ** 0.5), _bf(torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5)
    b1, b2 = (0.1 * torch.randn(4 * C, generator=g)).float().double(), (0.1 * torch.randn(C, generator=g)).float().double()
    gamma, beta, sc = _norm_randn(g, M, C)
    u = x @ W1.T + b1[None]
    h = gelu_erf64(u)
    y = h @ W2.T + b2[None]
    dy, dh = dy_mlp(C, x.abs() @ W1.abs().T + b1.abs()[None], h, W2, b2)
    ref, bo, bt = out_bound("mlp", y, dy, gamma, beta, sc, C)
    return dict(kernel="mlp", x=x, W1=W1, b1=b1, W=W2, b=b2, gamma=gamma, beta=beta, sc=sc, u=u, h=h, y=y, dy=dy, ref=ref, bound=bo, bound_t=bt, C=C)


SWEEP_M = 129  # 64 bands of u, twice, and one ragged row of a second workgroup


@functools.lru_cache(maxsize=None)
def mlp_sweep(C, M=SWEEP_M):
    """`mlp` with the hidden layer laid bare, so that the Level 2 expression is tight where the polynomial works: sweep channel
    c < C / 2 listens to ONE hidden unit n(c) = c + C (c mod 4), which listens to x column c alone with weight 1 and bias
    (c mod 4) / 64: u = x + b1 is one exact f32 addition and y_c = h(u) with delta_y = 1.2e-4 + 2^-8 |h| (+ a g term of 1e-6).  Row
    r sweeps the band a_r + {0 .. 11} / 64 with a_r = -6 + 3 (r mod 64) / 16: every multiple of 1/64 in [-6, 6) is met.  The other
    half of the channels are anchors y = +-1 from the bias alone, so that the row has a variance of its own and an error shared by a
    whole band is not taken out again by the mean."""
    g = gen(9900 + C)
    HD = 4 * C
    r, c = torch.arange(M), torch.arange(C)
    x = (-6.0 + 3.0 * (r % 64)[:, None] / 16.0 + ((c // 4) % 3)[None, :] / 16.0).double()
    W1 = torch.zeros(HD, C, dtype=torch.float64)
    n = torch.arange(HD)
    W1[n, n % C] = 1.0
    b1 = (n // C).double() / 64.0
    W2 = torch.zeros(C, HD, dtype=torch.float64)
    half = torch.arange(C // 2)
    listens = half + C * (half % 4)
    W2[half, listens] = 1.0
    b2 = torch.zeros(C, dtype=torch.float64)
    b2[C // 2:] = 1.0 - 2.0 * (torch.arange(C // 2) % 2)
    gamma, beta, sc = _norm_randn(g, M, C)
    u = x @ W1.T + b1[None]
    h = gelu_erf64(u)
    y = h @ W2.T + b2[None]
    dy, dh = dy_mlp(C, x.abs() @ W1.abs().T + b1.abs()[None], h, W2, b2)
    ref, bo, bt = out_bound("mlp", y, dy, gamma, beta, sc, C)
    return dict(kernel="mlp", x=x, W1=W1, b1=b1, W=W2, b=b2, gamma=gamma, beta=beta, sc=sc, u=u, h=h, y=y, dy=dy, ref=ref, bound=bo, bound_t=bt, C=C,
                listens=listens)


RANDN_ROW_KEYS = ("x", "sc", "u", "h", "y", "dy", "ref", "bound", "bound_t")


def take_randn_rows(fx, M):
    return {k: (v[:M] if k in RANDN_ROW_KEYS else v) for k, v in fx.items()}


def reference_randn(fx, **moved):
    """fp64 output of a randn case with operands replaced (the shifted-index check)"""
    o = {**fx, **moved}
    a = gelu_erf64(o["x"] @ o["W1"].T + o["b1"][None]) if fx["kernel"] == "mlp" else o["x"]
    y = a @ o["W"].T + o["b"][None]
    d = y - y.mean(-1, keepdim=True)
    return d * (d.pow(2).mean(-1, keepdim=True) + EPS).rsqrt() * o["gamma"][None] + o["beta"][None] + o["sc"]
