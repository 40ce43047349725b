"""float64 / exact reference of gradient-norm clipping (optim.clip_grad_norm_, csrc/grad_clip.hip) in numpy.

L2: every fp32 value's square is exact in float64 (24 + 24 significant bits), and math.fsum adds them without error, so
`sq_sum` is the correctly rounded sum of squares whatever the length.  inf: the maximum of |g| with NaN propagation (numpy's
max propagates NaN).  The coefficient and the scaled gradients repeat the fp32 arithmetic of torch.nn.utils.clip_grad_norm_:
c = max_norm / (total + 1e-6), clamp(max = 1) that keeps NaN, g * coef."""
import math

import numpy as np

INF = float("inf")


def sq_sum(g):
    """correctly rounded float64 sum of the squares of a float array"""
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    sq = g * g
    if not np.all(np.isfinite(sq)):
        return float("nan") if np.any(np.isnan(sq)) else INF
    return math.fsum(sq.tolist())


def max_abs(g):
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    return float(np.max(np.abs(g))) if g.size else 0.0


def norms(grads, norm_type=2.0):
    """(per-tensor norms, total) as float64"""
    if float(norm_type) == INF:
        per = [max_abs(g) for g in grads]
        total = float(np.max(np.array(per))) if per else 0.0  # np.max keeps NaN
        return per, total
    assert float(norm_type) == 2.0
    s = [sq_sum(g) for g in grads]
    bad = [x for x in s if not math.isfinite(x)]
    if bad:
        tot = float("nan") if any(math.isnan(x) for x in bad) else INF
    else:
        tot = math.fsum(s)
    return [math.sqrt(x) if x == x else x for x in s], (math.sqrt(tot) if tot == tot else tot)


def total_sq(grads):
    """the exact-as-float64 sum of all squares (L2 only): for tests that need S itself"""
    return math.fsum(sq_sum(g) for g in grads)


def coef(total, max_norm):
    """the fp32 coefficient from a total norm: every step rounded to float32 as the kernel and torch do"""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(total) + np.float32(1e-6))
    if c < 1:
        return np.float32(c)
    return np.float32(1.0) if c >= 1 else np.float32(c)  # NaN stays


def scaled(grads, c):
    """expected gradients: float32(g) * float32(coef), one rounding per element"""
    with np.errstate(all="ignore"):
        return [np.asarray(g, dtype=np.float32) * np.float32(c) for g in grads]


def clip(grads, max_norm, norm_type=2.0):
    """(total float64, coef float32, scaled gradients) of one clip_grad_norm_ call on fp32 gradients"""
    _per, total = norms(grads, norm_type)
    c = coef(total, max_norm)
    return total, c, scaled(grads, c)


def ulp32(x):
    """spacing of float32 at |x|"""
    return float(np.spacing(np.abs(np.float32(x))))


def within_ulps(got, want, n=1):
    """|got - float32(want)| <= n float32 ulps (at want); equal NaNs / infinities count as within"""
    got, w32 = np.float32(got), np.float32(want)
    if np.isnan(w32) or np.isnan(got):
        return bool(np.isnan(w32) and np.isnan(got))
    if np.isinf(w32) or np.isinf(got):
        return bool(got == w32)
    return abs(float(got) - float(w32)) <= n * ulp32(w32)
