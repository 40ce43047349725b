"""fp64 reference, fixtures and per-element bounds of the cross-entropy with knowledge distillation (csrc/ce.hip) for
tests/test_distill_cpu.py and tests/test_distill_gpu.py.

    ce      = loss_opts_ref's l                                                              (label smoothing eps, z-loss z)
    p       = softmax(t / T),  q = softmax(x / T),   kl = sum_j p_j (log p_j - log q_j)
    l       = (1 - alpha) ce + alpha T^2 kl                                                  (0 where y == -100)
    loss    = sum_i w_i l_i / W
    dl/dx_j = (w_i / W) [ (1 - alpha) (loss_opts_ref's bracket) + alpha T (q_j - p_j) ]

The student fixtures are tests/rowops_ref.py::ce_case's and loss_opts_ref's weights; the teacher is 0.7 x + 2 randn with one -150
and one +15 per row, as its dtype stores it.  The reference is computed from the stored operands.

Bounds: first-order worst case, FACTOR = 1, u = 2^-24.  They are loss_opts_ref's for the cross-entropy part (taken from there,
unchanged: the kernel computes that part by the same operations) with the roundings of what the kernel adds.  The kernel evaluates,
with a_j = (t_j - max t) / T, b_j = (x_j - max x) / T, st = sum_j exp(a_j), sq = sum_j exp(b_j), D = sum_j exp(a_j) (t_j - x_j):

    kl = (((D / st) - (max t - max x)) / T - log st) + log sq

  exp(a_j)             the argument carries three roundings (the difference, 1 / T, the product): 3 u |a_j|; __expf's model is
                       expf_rel.  The two-pass form (online soft-max) reaches the value through a chain of at most
                       ceil(V / (256 VEC)) + 2 factors exp(.) whose arguments add up to a_j, the one-pass form through one:
                       relE(a) = u (2 |a| + 4 chain) + 3 u |a| + 2 u (chain - 1)
  a sum over the row   a lane adds (VEC + 1) ceil(V / (256 VEC)) values (the vector's partial sum joins the running one), the wave
                       folds 6 times, four waves merge with 3 adds, one more for the fused join: A = that + 10 roundings
  st, sq               rel(st) = sum_j p_j relE(a_j) + A u, rel(sq) likewise with q and b
  log st, log sq       rel(st) through the derivative plus ce_case's allowance for __logf and what surrounds it, u (2 |log st| + 16)
  S = D / st           each product exp(a_j) d_j with d_j = t_j - x_j has relE(a_j) + 2 u (d_j rounds once, the product once), the sum
                       A u: sum_j p_j |d_j| (relE(a_j) + (A + 2) u); the quotient |S| (rel(st) + 3 u)
  the assembly of kl   c = max t - max x rounds once; S - c once; 1 / T and the product once each; the two logarithms join with a
                       rounding each: (u |c| + 3 u |S - c|) / T + u |(S - c) / T - log st| + u |kl|
  l                    1 - alpha rounds once and multiplies ce (2 more with the join), alpha T^2 carries two roundings and multiplies
                       kl (2 more): u (3 |(1 - alpha) ce| + 4 |alpha T^2 kl|) + u |l| on top of (1 - alpha) dce + alpha T^2 dkl
  q_j and p_j          the gradient pass evaluates q_j = exp(x_j / T - lq) with lq = max x / T + log sq (at T == 1 the cross-entropy's
                       exp(x_j - lse), the same form): the argument's error is 3 u |x_j / T| + u |arg| + dlq with
                       dlq = 2 u |max x / T| + dlog sq + u |lq|; p_j the same from t
  the gradient         alpha (g T) (q_j - p_j): the difference rounds once, the coefficient three times beside the error of g
                       ((rows + 3) u, loss_opts_ref); the join (1 - alpha) A + that rounds the first product and the sum:
                       u (2 |(1 - alpha) A| + |second term|) + u |grad|
  bf16 store           2^-8 |grad|; 2^-120 absolute for what underflows in f32 (loss_opts_ref's floor)"""
import functools
import math

import torch

from tests import loss_opts_ref as LR
from tests.exact_ref import U8, U24, gen
from tests.rowops_ref import ce_case, expf_rel

FACTOR = 1.0  # the bounds below are used as derived
SETTINGS = ((0.5, 1.0), (1.0, 2.0), (0.3, 0.5))  # (alpha, T)
OPTIONS = ((0.0, 0.0), (0.3, 0.05))              # (eps, z)
TDTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}


def reference(x, t, labels, eps=0.0, z=0.0, weights=None, alpha=0.5, T=1.0):
    """fp64: loss_opts_ref.reference's dict for the combined loss, with kl_row, p and q beside it (ce_row, ce_grad: the parts)"""
    r = LR.reference(x, labels, eps, z, weights)
    x, t = x.double(), t.double()
    lp, lq = torch.log_softmax(t / T, -1), torch.log_softmax(x / T, -1)
    p, q = lp.exp(), lq.exp()
    kl = (p * (lp - lq)).sum(-1)
    valid, g = r["valid"], r["g"]
    kl_row = torch.where(valid, kl, torch.zeros_like(kl))
    loss_row = torch.where(valid, (1.0 - alpha) * r["loss_row"] + alpha * T * T * kl, torch.zeros_like(kl))
    w = torch.ones(x.shape[0], dtype=torch.float64) if weights is None else weights.double()
    grad = (1.0 - alpha) * r["grad"] + g[:, None] * (alpha * T) * (q - p)
    return dict(r, ce_row=r["loss_row"], ce_grad=r["grad"], kl_row=kl_row, loss_row=loss_row, loss=r["inv_w"] * float((w * loss_row).sum()),
                grad=grad, pt=p, qt=q)


def torch_loss(logits, teacher, labels, eps=0.0, z=0.0, weights=None, alpha=0.5, T=1.0):
    """the formula as a direct differentiable torch expression in the dtype of `logits` ([rows, V]): cross_entropy's parts from
    loss_opts_ref.torch_loss's expression, the soft term from torch.nn.functional.kl_div(log_target=True)"""
    import torch.nn.functional as F
    rows, V = logits.shape
    valid = labels != -100
    lse = torch.logsumexp(logits, -1)
    xy = logits[torch.arange(rows), labels.clamp_min(0)]
    ce = lse - (1.0 - eps) * xy - (eps / V) * logits.sum(-1) + z * lse * lse
    kl = F.kl_div(torch.log_softmax(logits / T, -1), torch.log_softmax(teacher.to(logits.dtype) / T, -1), reduction="none", log_target=True).sum(-1)
    l = (1.0 - alpha) * ce + alpha * T * T * kl
    w = torch.ones(rows, dtype=logits.dtype) if weights is None else weights.to(logits.dtype)
    w = torch.where(valid, w, torch.zeros_like(w))
    W = w.sum()
    if float(W) == 0.0:
        return (l * 0.0).sum()
    return (w * l).sum() / W


@functools.lru_cache(maxsize=None)
def teacher_for(rows, V, dt, tdt):
    """the teacher's logits as `tdt` stores them ([rows, V]); finite"""
    c = ce_case(rows, V, dt)
    g = gen(7800 + V + rows)
    t = 0.7 * c["stored"].float() + 2.0 * torch.randn(rows, V, generator=g)
    cols = torch.stack([torch.randperm(V, generator=g)[:2] for _ in range(rows)])
    t[torch.arange(rows), cols[:, 0]] = -150.0
    t[torch.arange(rows), cols[:, 1]] = 15.0
    return t.to(TDTYPE[tdt])


def one_pass(V, dt):
    """the dispatch of csrc/ce.hip"""
    return dt == "bf16" and V <= 32768


def bounds(x, t, labels, dt, eps, z, w32, alpha, T, ce):
    """x, t: the stored operands in fp64; ce: loss_opts_ref.opts_case's dict of the same student, labels and options.  Returns the
    reference (reference()'s dict) and kl_bound, row_bound, gbound, loss_bound."""
    rows, V = x.shape
    r = reference(x, t, labels, eps, z, w32, alpha, T)
    valid = r["valid"]
    vec = 8 if dt == "bf16" else 4
    iters = math.ceil(V / (256 * vec))
    chain = 1 if one_pass(V, dt) else iters + 2
    A = (vec + 1) * iters + 10
    invT = 1.0 / T
    bm, tm = x.amax(-1, keepdim=True), t.amax(-1, keepdim=True)
    a, b = (t - tm) * invT, (x - bm) * invT
    p, q = r["pt"], r["qt"]

    def relE(v):
        return U24 * (2.0 * v.abs() + 4.0 * chain) + 3.0 * U24 * v.abs() + 2.0 * U24 * (chain - 1)

    rel_st, rel_sq = (p * relE(a)).sum(-1) + A * U24, (q * relE(b)).sum(-1) + A * U24
    lst, lsq = torch.logsumexp(a, -1), torch.logsumexp(b, -1)
    dlst, dlsq = rel_st + U24 * (2.0 * lst.abs() + 16.0), rel_sq + U24 * (2.0 * lsq.abs() + 16.0)
    d = t - x
    S = (p * d).sum(-1)
    dS = (p * d.abs() * (relE(a) + (A + 2) * U24)).sum(-1) + S.abs() * (rel_st + 3.0 * U24)
    c = (tm - bm)[:, 0]
    kl = (p * (torch.log_softmax(t / T, -1) - torch.log_softmax(x / T, -1))).sum(-1)
    dkl = (invT * dS + invT * U24 * (c.abs() + 3.0 * (S - c).abs()) + dlst + dlsq + U24 * ((S - c) * invT - lst).abs() + U24 * kl.abs())
    kl_bound = FACTOR * torch.where(valid, dkl, torch.zeros_like(dkl))
    oma, aT2 = 1.0 - alpha, alpha * T * T
    row_bound = (oma * ce["row_bound"] + aT2 * dkl + U24 * (3.0 * (oma * r["ce_row"]).abs() + 4.0 * (aT2 * kl).abs()) + U24 * r["loss_row"].abs())
    row_bound = FACTOR * torch.where(valid, row_bound, torch.zeros_like(row_bound))
    # the gradient
    wd = torch.ones(rows, dtype=torch.float64) if w32 is None else w32.double()
    live = valid & (wd > 0)
    g = r["g"]
    grel = (rows + 3) * U24
    lq, lt = bm[:, 0] * invT + lsq, tm[:, 0] * invT + lst
    dlq = 2.0 * U24 * (bm[:, 0] * invT).abs() + dlsq + U24 * lq.abs()
    dlt = 2.0 * U24 * (tm[:, 0] * invT).abs() + dlst + U24 * lt.abs()
    argq, argp = x * invT - lq[:, None], t * invT - lt[:, None]
    relq = expf_rel(argq) + 3.0 * U24 * (x * invT).abs() + U24 * argq.abs() + dlq[:, None]
    relp = expf_rel(argp) + 3.0 * U24 * (t * invT).abs() + U24 * argp.abs() + dlt[:, None]
    dqp = q * relq + p * relp + U24 * (q - p).abs()
    second = (alpha * T) * g[:, None] * (q - p)
    dsecond = (alpha * T) * g[:, None] * (dqp + (grel + 3.0 * U24) * (q - p).abs())
    dA = ce["gbound"] - (U8 * ce["grad"].abs() if dt == "bf16" else 0.0)  # the cross-entropy's element before the store
    gbound = oma * dA + dsecond + U24 * (2.0 * (oma * r["ce_grad"]).abs() + second.abs()) + U24 * r["grad"].abs() + 2.0 ** -120
    if dt == "bf16":
        gbound = gbound + U8 * r["grad"].abs()
    gbound = FACTOR * torch.where(live[:, None], gbound, torch.zeros_like(x))
    wl = wd * r["loss_row"]
    loss_bound = FACTOR * r["inv_w"] * ((wd * row_bound).sum() + (2 * (rows / 256 + 12) + rows + 4) * U24 * wl.abs().sum())
    return r, dict(kl_bound=kl_bound, row_bound=row_bound, gbound=gbound, loss_bound=loss_bound)


@functools.lru_cache(maxsize=None)
def distill_case(rows, V, dt, tdt, eps, z, weighted, alpha, T, same=False):
    """loss_opts_ref.opts_case(rows, V, dt, eps, z, weighted) distilled from teacher_for(rows, V, dt, tdt) -- or, with `same`, from
    the student's own stored logits in the teacher's dtype -- at (alpha, T).  Cached: callers must not write into it."""
    ce = LR.opts_case(rows, V, dt, eps, z, weighted)
    teacher = ce["stored"].to(TDTYPE[tdt]) if same else teacher_for(rows, V, dt, tdt)
    x, t = ce["stored"].double(), teacher.double()
    if same:
        assert torch.equal(x, t)  # (bf16 logits in an f32 teacher and back: the same values)
    r, b = bounds(x, t, ce["labels"], dt, eps, z, ce["weights"], alpha, T, ce)
    return dict(stored=ce["stored"], teacher=teacher, labels=ce["labels"], valid=ce["valid"], dtype=ce["dtype"], weights=ce["weights"],
                loss_row=r["loss_row"], kl_row=r["kl_row"], grad=r["grad"], ce_grad=r["ce_grad"], loss=torch.tensor(r["loss"], dtype=torch.float64),
                inv_w=ce["inv_w"], inv_w_bound=ce["inv_w_bound"], **b)


def teacher_vector(tdt):
    """elements of the teacher's 16-byte vector: widths and strides off it are refused"""
    return 8 if tdt == "bf16" else 4
