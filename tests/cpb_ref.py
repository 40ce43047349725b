"""Fixtures, fp64 reference and per-element bounds for the Swin-V2 continuous-position-bias kernels (cpb_table_kernel,
cpb_gather_kernel, cpb_dtable_kernel, cpb_mlp_bwd_kernel in csrc/attn_swin.hip; cpb_sigmoid_kernel, cpb_dtable_from_btab_kernel,
cpb_mlp_bwd_any_kernel in csrc/attn_swin_large.hip): plain torch on the CPU, shared by tests/test_cpb_fixtures_cpu.py and
tests/test_cpb_exact_gpu.py.

Reference (HF/swinv2:376-378, 418-428 and its gradient), fp64 from the f32 inputs:
    hidden = relu(coords W0^T + b0)   [ntab, nh]        table = hidden W2^T   [ntab, H]        btab = 16 sigmoid(table)
    bias[h, ij] = btab[index[ij], h]                                                            (dense form)
    dtable[t, h] = sum_{ij: index[ij] = t} dbias[h, ij] b (1 - b / 16),  b = bias[h, ij]        (table form: dbtab[t, h] b (1 - b / 16))
    dW2[h, j] = sum_t dtable[t, h] hidden[t, j]
    g[t, j]   = [hidden[t, j] > 0] sum_h dtable[t, h] W2[h, j]           the gate reads the f32 hidden handed to the kernel
    dW0[j, :] = sum_t g[t, j] coords[t, :]          db0[j] = sum_t g[t, j]

Exact forward fixture: coords and b0 are multiples of 1/8 in [-1, 1], W0 integers in [-2, 2]: every pre-activation is a multiple of
1/8 of magnitude <= 5, many exactly 0 and many negative; W2 integers in [-3, 3], so a table entry is a sum of at most 512 multiples of
1/8 whose absolute values add up to less than 2^17 units: exact in any order.

Exact backward fixture (every operand is an input): btab in {0, 4, 8, 12, 16}, where b (1 - b / 16) is 0, 3, 4, 3, 0 without rounding;
bias its gather; dbias integers in [-2, 2], about 70 % zeros; hidden integers in [0, 3], about a third zeros; W2 integers in [-2, 2];
coords multiples of 1/8.  Every output is then a sum of integers (multiples of 1/8 for dW0); tests/test_cpb_fixtures_cpu.py adds up
the absolute values of the terms of every output element, the initial content included, and demands less than 2^24 units, which
makes the result independent of the order of the atomics and of the reductions.

Bounds (first order, u = 2^-24, nothing measured).
  forward:  e_hid = 3 u (|w00 c0| + |w01 c1| + |b0|)        two products, two additions (ReLU is 1-Lipschitz)
            e_tab = sum_j e_hid_j |W2_hj| + 12 u sum_j |hid_j W2_hj|     at most 2 terms per thread, 6 shuffle levels, 3 additions, products
            e_b   = b (1 - b / 16) (e_tab + u (2 |table| + 4)) + 3 u b   the slope of 16 sigmoid, the project's model of __expf
                                                                         (swin_exact_ref.SwinBounds), the addition, the division
  backward: e_dt[t, h] = u (3 + cnt_t) sum |terms|                        three roundings per term, cnt_t atomic additions in any order
            e_dW2 = sum_t e_dt |hid| + 32 u (sum_t |dt hid| + |init|)     12 in-thread terms, 16 partial sums, the products, the add-to
            e_g   = sum_h e_dt |W2| + (H + 1) u sum_h |dt W2|
            e_dW0 = sum_t e_g |c| + 32 u (sum_t |g c| + |init|),  e_db0 likewise without c"""
import functools
import math

import torch

U24 = 2.0 ** -24
FWD_W = (2, 4, 7, 8)
FWD_H = (1, 3, 32)
FWD_NH = (40, 300, 512)
REAL_WINDOWS = ((2, 0), (4, 0), (7, 0), (8, 0), (8, 6), (4, 7))  # (w, pretrained w); 0: the window itself
# backward exact cases: (ntab, n, real index?)
BWD_CASES = ((9, 4, True), (49, 16, True), (169, 49, True), (192, 49, False), (193, 49, False), (225, 64, True))
BWD_H_LDS = (1, 3, 4, 24, 32)
BWD_H_ANY = (1, 8, 64)
BWD_NH = (40, 512)
MUTATIONS = ("gate_ge", "index_transposed", "last_row_dropped", "heads_ge16_dropped", "dw0_swapped", "tail_units_dropped", "dtable_not_cleared")


def bwd_exact_cases():
    """(ntab, n, real, H, nh): every H of its form at every table size, both hidden widths"""
    return [(ntab, n, real, H, nh) for ntab, n, real in BWD_CASES for H in (BWD_H_LDS if ntab <= 192 else BWD_H_ANY) for nh in BWD_NH]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def real_tables(w, pw):
    """coords [ntab, 2] f32 and index [n * n] int32 as the engine builds them"""
    from klab_multimodalmodel_amd.engine import swin_cpb_tables
    return swin_cpb_tables(w, pw)


def dyadic_coords(ntab):
    t = torch.arange(ntab)
    return torch.stack([((t % 17) - 8) / 8.0, ((5 * t + 3) % 17 - 8) / 8.0], 1).double()


# ---- reference ---------------------------------------------------------------------------------------------------------------------
def forward(coords, w0, b0, w2):
    pre = coords @ w0.T + b0[None]
    hidden = pre.clamp_min(0.0)
    table = hidden @ w2.T
    return dict(pre=pre, hidden=hidden, table=table, btab=16.0 * torch.sigmoid(table))


def dense(btab, index, n):
    """[ntab, H] -> [H, n * n]"""
    return btab[index.long()].T.contiguous()


def dtable_dense(dbias, bias, index, ntab, transposed=False):
    """[H, n * n] x 2 -> dtable [ntab, H] and the sum of the terms' absolute values"""
    nn = index.numel()
    n = int(round(math.sqrt(nn)))
    ix = index.long().view(n, n).T.reshape(-1) if transposed else index.long()
    term = (dbias * bias * (1.0 - bias * 0.0625)).T  # [nn, H]
    z = torch.zeros(ntab, dbias.shape[0], dtype=torch.float64)
    return z.clone().index_add_(0, ix, term), z.clone().index_add_(0, ix, term.abs())


def mlp_backward(dtable, coords, hidden, w2, mut=None):
    """dW0 [nh, 2], db0 [nh], dW2 [H, nh] (without the initial content) and the sums of absolute values of their terms"""
    ntab, nh = hidden.shape
    dt = dtable
    if mut == "last_row_dropped":
        dt = dtable.clone()
        dt[ntab - 1] = 0.0
    gate = (hidden >= 0) if mut == "gate_ge" else (hidden > 0)
    dw2 = dt.T @ hidden
    g = (dt @ w2) * gate
    ga = (dt.abs() @ w2.abs()) * gate
    dw0, db0 = g.T @ coords, g.sum(0)
    out = dict(dw0=dw0, db0=db0, dw2=dw2, g=g, abs_dw2=dt.abs().T @ hidden.abs(), abs_g=ga, abs_dw0=ga.T @ coords.abs(), abs_db0=ga.sum(0))
    if mut == "heads_ge16_dropped":
        out["dw2"] = dw2.clone()
        out["dw2"][16:] = 0.0
    if mut == "dw0_swapped":
        out["dw0"] = dw0.flip(1)
    if mut == "tail_units_dropped":
        cut = nh // 16 * 16
        for k in ("dw0", "db0"):
            out[k] = out[k].clone()
            out[k][cut:] = 0.0
        out["dw2"] = out["dw2"].clone()
        out["dw2"][:, cut:] = 0.0
    return out


def backward(fx, mut=None, dtable0=None):
    """the four outputs of klab_swin_cpb_bias_bwd_pz on fixture fx, initial contents included.  dtable0: what dtable holds when the
    scatter starts (None: cleared; the mutation dtable_not_cleared starts from the NaN the test puts there)"""
    dt, dta = dtable_dense(fx.dbias, fx.bias, fx.index, fx.ntab, transposed=mut == "index_transposed")
    if mut == "dtable_not_cleared":
        dtable0 = torch.full_like(dt, float("nan"))
    if dtable0 is not None:
        dt, dta = dt + dtable0, dta + dtable0.abs()
    m = mlp_backward(dt, fx.coords, fx.hidden, fx.w2, mut)
    return dict(dtable=dt, dw0=m["dw0"] + fx.init["dw0"], db0=m["db0"] + fx.init["db0"], dw2=m["dw2"] + fx.init["dw2"], abs_dtable=dta,
                abs_dw0=m["abs_dw0"] + abs(fx.init["dw0"]), abs_db0=m["abs_db0"] + abs(fx.init["db0"]),
                abs_dw2=m["abs_dw2"] + abs(fx.init["dw2"]), parts=m)


OUTPUTS = ("dtable", "dw0", "db0", "dw2")
INIT = dict(dw0=5.0, db0=-3.0, dw2=7.0)  # accumulated outputs start from non-zero integers


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
class Fx:
    pass


@functools.lru_cache(maxsize=None)
def fwd_exact_fixture(w, H, nh):
    """synthetic dyadic MLP over the real index of window w"""
    g = gen(4000 + 100 * w + 10 * H + nh)
    _, index = real_tables(w, 0)
    fx = Fx()
    fx.ntab, fx.n, fx.H, fx.nh, fx.index = (2 * w - 1) ** 2, w * w, H, nh, index
    fx.coords = dyadic_coords(fx.ntab)
    fx.w0, fx.b0, fx.w2 = ints(g, -2, 2, nh, 2), ints(g, -8, 8, nh) / 8.0, ints(g, -3, 3, H, nh)
    fx.ref = forward(fx.coords, fx.w0, fx.b0, fx.w2)
    return fx


@functools.lru_cache(maxsize=None)
def fwd_random_fixture(w, pw, H, nh):
    g = gen(5000 + 100 * w + 17 * pw + 10 * H + nh)
    coords, index = real_tables(w, pw)
    fx = Fx()
    fx.ntab, fx.n, fx.H, fx.nh, fx.index = (2 * w - 1) ** 2, w * w, H, nh, index
    fx.coords = coords.double()
    fx.w0 = torch.randn(nh, 2, generator=g).double()
    fx.b0 = torch.randn(nh, generator=g).double()
    fx.w2 = (torch.randn(H, nh, generator=g) * (2.0 / math.sqrt(nh))).double()
    fx.ref = forward(fx.coords, fx.w0, fx.b0, fx.w2)
    return fx


def fwd_bounds(fx):
    """e_hid [ntab, nh], e_tab [ntab, H], e_b [ntab, H]"""
    r = fx.ref
    e_hid = 3.0 * U24 * (fx.coords[:, :1].abs() * fx.w0[None, :, 0].abs() + fx.coords[:, 1:].abs() * fx.w0[None, :, 1].abs() + fx.b0[None].abs())
    e_tab = e_hid @ fx.w2.abs().T + 12.0 * U24 * (r["hidden"].abs() @ fx.w2.abs().T)
    b = r["btab"]
    e_b = b * (1.0 - b / 16.0) * (e_tab + U24 * (2.0 * r["table"].abs() + 4.0)) + 3.0 * U24 * b
    return e_hid, e_tab, e_b


@functools.lru_cache(maxsize=None)
def bwd_exact_fixture(ntab, n, real, H, nh):
    g = gen(6000 + 7 * ntab + 3 * H + nh)
    fx = Fx()
    fx.ntab, fx.n, fx.H, fx.nh = ntab, n, H, nh
    if real:
        w = int(round(math.sqrt(n)))
        assert (2 * w - 1) ** 2 == ntab
        fx.index = real_tables(w, 0)[1]
    else:  # any value of [0, ntab), the last row among them
        fx.index = torch.randint(0, ntab, (n * n,), generator=g).to(torch.int32)
        fx.index[n * n // 2] = ntab - 1
    fx.coords = dyadic_coords(ntab)
    fx.btab = 4.0 * ints(g, 0, 4, ntab, H)
    fx.btab[ntab - 1] = 4.0 * (1 + torch.arange(H) % 3)  # the last row's slope is never 0
    fx.bias = dense(fx.btab, fx.index, n)
    keep = torch.rand(H, n * n, generator=g) < 0.3
    fx.dbias = ints(g, -2, 2, H, n * n) * keep
    last = (fx.index.long() == ntab - 1).nonzero().flatten()
    fx.dbias[:, last[0]] = 1.0 + torch.arange(H) % 2  # ... and its gradient is not 0 either
    fx.dbias[:, last[1:]] = 0.0
    hid = ints(g, 1, 3, ntab, nh) * (torch.rand(ntab, nh, generator=g) < 0.67)
    hid[ntab - 1] = 1.0 + torch.arange(nh) % 3
    hid[ntab - 1, ::5] = 0.0
    fx.hidden = hid
    fx.w2 = ints(g, -2, 2, H, nh)
    fx.init = INIT
    fx.dbtab = torch.zeros(ntab, H, dtype=torch.float64).index_add_(0, fx.index.long(), fx.dbias.T.contiguous())
    return fx


@functools.lru_cache(maxsize=None)
def bwd_random_dbias(H, nn, seed):
    return torch.randn(H, nn, generator=gen(7000 + seed)).double()


def bwd_bounds(fx, r):
    """per-element bounds of the four outputs from the fp64 result r = backward(fx)"""
    cnt = torch.zeros(fx.ntab, dtype=torch.float64).index_add_(0, fx.index.long(), torch.ones(fx.index.numel(), dtype=torch.float64))
    e_dt = U24 * (3.0 + cnt[:, None]) * r["abs_dtable"]
    hid, w2, c = fx.hidden.abs(), fx.w2.abs(), fx.coords.abs()
    gate = (fx.hidden > 0).double()
    e_dw2 = e_dt.T @ hid + 32.0 * U24 * r["abs_dw2"]
    e_g = ((e_dt @ w2) + (fx.H + 1.0) * U24 * (r["dtable"].abs() @ w2)) * gate
    e_dw0 = e_g.T @ c + 32.0 * U24 * r["abs_dw0"]
    e_db0 = e_g.sum(0) + 32.0 * U24 * r["abs_db0"]
    return dict(dtable=e_dt, dw0=e_dw0, db0=e_db0, dw2=e_dw2)


BWD_RANDOM = ((2, 0, 3, 40), (4, 0, 4, 512), (7, 0, 24, 40), (7, 0, 3, 512), (8, 0, 8, 512), (8, 6, 64, 40), (4, 7, 32, 300))  # (w, pw, H, nh)


def bwd_random_fixture(w, pw, H, nh, hidden=None, bias=None):
    """real coords and index, random dbias; hidden [ntab, nh] and bias [H, n * n] as the forward kernel stored them (f32 values in
    fp64), or, without a GPU, the fp64 forward rounded to f32"""
    f = fwd_random_fixture(w, pw, H, nh)
    fx = Fx()
    fx.ntab, fx.n, fx.H, fx.nh, fx.index, fx.coords, fx.w2 = f.ntab, f.n, H, nh, f.index, f.coords, f.w2
    fx.hidden = f.ref["hidden"].float().double() if hidden is None else hidden
    fx.bias = dense(f.ref["btab"], f.index, f.n).float().double() if bias is None else bias
    fx.dbias = bwd_random_dbias(H, f.n * f.n, 100 * w + pw).clone()
    last = (f.index.long() == f.ntab - 1).nonzero().flatten()
    fx.dbias[:, last] = 8.0 * torch.sign(fx.dbias[:, last])  # table row ntab - 1 has one entry: its gradient is not small
    fx.init = INIT
    return fx
