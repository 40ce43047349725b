"""fp64 reference, fixtures and per-element bounds of the cross-entropy with options (csrc/ce.hip) for
tests/test_loss_opts_cpu.py and tests/test_loss_opts_gpu.py.

    l_i     = lse - (1 - eps) x_y - (eps / V) sum_j x_j + z lse^2          (0 where y == -100)
    W       = sum of w_i over the rows with a label,   loss = sum_i w_i l_i / W      (0 when W == 0)
    dl/dx_j = (w_i / W) [ p_j (1 + 2 z lse) - (1 - eps) [j == y] - eps / V ]

The fixtures are tests/rowops_ref.py::ce_case's (logits 3 randn with one -200 and one +20 per row, the same label placement);
the weights are drawn from {0, 0.25, 1, 3} with a 0 forced onto one row with a label and a 3 onto one row without.

Bounds: first-order worst case, FACTOR = 1 (nothing is multiplied onto the derived terms).  They are ce_case's with the added
operations' roundings:
  dlse                 ce_case's term for the error of lse, unchanged (lse is computed by the same operations)
  sum_j x_j            a lane adds ceil(V / 2048) * 8 values (f32: ceil(V / 1024) * 4), the wave folds 6 times, four waves merge with 3
                       adds: (adds + 1) 2^-24 sum_j |x_j|, times eps / V
  z lse^2              two products and the sum: 3 2^-24 z lse^2 plus the error of lse through the derivative, 2 z |lse| dlse
  the sum of the row   four terms, each rounded when it joins: 4 2^-24 (|lse| + (1 - eps) |x_y| + (eps / V) |sum x| + z lse^2)
  w inv_w              inv_w is one division of the f32 sum of the weights (rows adds of non-negative numbers: rows 2^-24
                       relative), the product one more rounding: (rows + 3) 2^-24 relative on the factor g = w / W
  the gradient bracket p_j k with k = 1 + 2 z lse (3 roundings of k, and dlse through 2 z).  Off the label the kernel evaluates
                       p_j (g k) - g (eps / V) -- the two coefficients round once each, the fused multiply-add once, eps / V
                       carries two roundings of its own; the label's element is ((p_y k - (1 - eps)) - eps / V) g, a rounding
                       per operation and those of the two constants: at most 6 2^-24 of the sum of the absolute terms either way
  bf16 store           2^-8 |grad|"""
import functools
import math

import torch

from tests.exact_ref import U8, U24, gen
from tests.rowops_ref import ce_case, expf_rel

FACTOR = 1.0  # the bounds below are used as derived
WEIGHT_VALUES = (0.0, 0.25, 1.0, 3.0)


def reference(x, labels, eps=0.0, z=0.0, weights=None):
    """fp64: dict(lse, p, loss_row, W, inv_w, loss, grad) of logits x [rows, V] (any float dtype), labels [rows], weights [rows] or None"""
    x = x.double()
    rows, V = x.shape
    w = torch.ones(rows, dtype=torch.float64) if weights is None else weights.double()
    valid = labels != -100
    lse = torch.logsumexp(x, -1)
    p = (x - lse[:, None]).exp()
    safe = labels.clamp_min(0)
    xy = x[torch.arange(rows), safe]
    l = lse - (1.0 - eps) * xy - (eps / V) * x.sum(-1) + z * lse * lse
    loss_row = torch.where(valid, l, torch.zeros_like(l))
    W = float((w * valid).sum())
    inv_w = 1.0 / W if W > 0 else 0.0
    delta = torch.zeros_like(x)
    delta[torch.arange(rows)[valid], labels[valid]] = 1.0
    g = torch.where(valid, w * inv_w, torch.zeros_like(w))
    grad = g[:, None] * (p * (1.0 + 2.0 * z * lse)[:, None] - (1.0 - eps) * delta - eps / V)
    return dict(lse=lse, p=p, loss_row=loss_row, W=W, inv_w=inv_w, loss=inv_w * float((w * loss_row).sum()), grad=grad, valid=valid, g=g)


@functools.lru_cache(maxsize=None)
def weights_for(rows, V):
    """f32 [rows] from WEIGHT_VALUES; a 0 on the first row with a label, a 3 on the first row without (where there is one)"""
    c = ce_case(rows, V, "f32" if V % 8 else "bf16")
    g = gen(7700 + V + rows)
    w = torch.tensor(WEIGHT_VALUES, dtype=torch.float32)[torch.randint(0, len(WEIGHT_VALUES), (rows,), generator=g)]
    valid = c["valid"]
    w[int(valid.nonzero()[0])] = 0.0
    if bool((~valid).any()):
        w[int((~valid).nonzero()[0])] = 3.0
    if float((w * valid).sum()) == 0.0:  # never all zero on the labelled rows
        w[int(valid.nonzero()[-1])] = 1.0
    return w


@functools.lru_cache(maxsize=None)
def opts_case(rows, V, dt, eps, z, weighted):
    """ce_case(rows, V, dt) under (eps, z, weights or None): the fp64 reference and the bounds.  Cached: callers must not write
    into it."""
    c = ce_case(rows, V, dt)
    x, lab, valid = c["stored"].double(), c["labels"], c["valid"]
    w32 = weights_for(rows, V) if weighted else None
    r = reference(x, lab, eps, z, w32)
    lse, p = r["lse"], r["p"]
    mx = x.amax(-1, keepdim=True)
    a = 8 * math.ceil(V / 2048) + 12
    dlse = ((p * expf_rel(x - mx)).sum(-1) + U24 * (a + 2 * lse.abs() + 16))  # ce_case's, per row
    lane_adds = 8 * math.ceil(V / 2048) if dt == "bf16" else 4 * math.ceil(V / 1024)
    sum_adds = lane_adds + 6 + 3 + 1
    sabs, ssum = x.abs().sum(-1), x.sum(-1)
    xy = x[torch.arange(rows), lab.clamp_min(0)]
    terms = lse.abs() + (1.0 - eps) * xy.abs() + (eps / V) * ssum.abs() + z * lse * lse
    row_bound = (dlse * (1.0 + 2.0 * z * lse.abs()) + (eps / V) * sum_adds * U24 * sabs + 3 * U24 * z * lse * lse + 4 * U24 * terms
                 + 2 * U24 * ((1.0 - eps) * xy.abs() + (eps / V) * ssum.abs()))  # (the last: the roundings of 1 - eps and eps / V)
    row_bound = FACTOR * torch.where(valid, row_bound, torch.zeros_like(row_bound))
    wd = torch.ones(rows, dtype=torch.float64) if w32 is None else w32.double()
    grel = (rows + 3) * U24  # relative error of g = w inv_w
    k = 1.0 + 2.0 * z * lse
    delta = torch.zeros_like(x)
    delta[torch.arange(rows)[valid], lab[valid]] = 1.0
    bracket = p * k[:, None] - (1.0 - eps) * delta - eps / V
    babs = p * k[:, None] + (1.0 - eps) * delta + eps / V
    dbr = (p * k[:, None] * (expf_rel(x - lse[:, None]) + dlse[:, None]) + p * (2.0 * z * dlse + 3 * U24 * k)[:, None] + 6 * U24 * babs)
    g = r["g"]
    gbound = g[:, None] * (dbr + (grel + U24) * bracket.abs()) + 2.0 ** -120
    if dt == "bf16":
        gbound = gbound + U8 * r["grad"].abs()
    gbound = FACTOR * torch.where((valid & (wd > 0))[:, None], gbound, torch.zeros_like(x))
    wl = wd * r["loss_row"]
    loss_bound = FACTOR * r["inv_w"] * ((wd * row_bound).sum() + (2 * (rows / 256 + 12) + rows + 4) * U24 * wl.abs().sum())
    return dict(stored=c["stored"], labels=lab, valid=valid, dtype=c["dtype"], weights=w32, loss_row=r["loss_row"], row_bound=row_bound,
                grad=r["grad"], gbound=gbound, loss=torch.tensor(r["loss"], dtype=torch.float64), loss_bound=loss_bound,
                inv_w=torch.tensor(r["inv_w"], dtype=torch.float64), inv_w_bound=torch.tensor((rows + 1) * U24 * r["inv_w"], dtype=torch.float64))


def torch_loss(logits, labels, eps=0.0, z=0.0, weights=None):
    """the formula as a direct differentiable torch expression in the dtype of `logits` ([rows, V]); labels and weights [rows]"""
    rows, V = logits.shape
    valid = labels != -100
    lse = torch.logsumexp(logits, -1)
    xy = logits[torch.arange(rows), labels.clamp_min(0)]
    l = lse - (1.0 - eps) * xy - (eps / V) * logits.sum(-1) + z * lse * lse
    w = torch.ones(rows, dtype=logits.dtype) if weights is None else weights.to(logits.dtype)
    w = torch.where(valid, w, torch.zeros_like(w))
    W = w.sum()
    if float(W) == 0.0:
        return (l * 0.0).sum()
    return (w * l).sum() / W
