"""Inputs, the fp64 reference and the per-element bounds for the fused AdamW kernel (csrc/adamw.hip), shared by
tests/test_adamw_cpu.py (which shows that an fp32 evaluation of the kernel's sequence stays inside the bounds) and
tests/test_adamw_gpu.py (which holds the kernel to them).  Plain torch / numpy on the CPU."""
import numpy as np
import torch

from tests import engine_kernels_ref as R
from tests.engine_kernels_ref import U24

MAX_GROUPS = 16
f32 = lambda a: float(np.float32(a))


def group(lr, beta1, beta2, eps, wd, step=3):
    """one klab_adamw_group as the f32 struct holds it: the bias corrections of update number `step`"""
    return dict(lr=f32(lr), beta1=f32(beta1), beta2=f32(beta2), eps=f32(eps), weight_decay=f32(wd),
                bias_corr1=f32(1 - f32(beta1) ** step), bias_corr2=f32(1 - f32(beta2) ** step))


# hyper-parameters of the existing Adam test (f32 holds lr, the betas and 1 - beta exactly), and a second learning rate that is not
# a power of two
BASE = dict(lr=2.0 ** -9, beta1=0.875, beta2=1 - 2.0 ** -10, eps=1e-8)


def one_group(wd, lr=BASE["lr"]):
    return [group(lr, BASE["beta1"], BASE["beta2"], BASE["eps"], wd)]


def three_groups():
    """different (lr, beta1, beta2, eps, wd) per group; group 2 has lr = 0 (and a decay that must then do nothing).  With tensors
    assigned i % 3, group 1 has no arena copies (the state's every third tensor) and group 2 has one for every tensor."""
    return [group(2.0 ** -9, 0.875, 1 - 2.0 ** -10, 1e-8, 0.01), group(3e-3, 0.9375, 0.96875, 1e-7, 0.0), group(0.0, 0.75, 1 - 2.0 ** -7, 1e-6, 0.1)]


ZERO_LR_GROUP = 2


def sixteen_groups():
    """sixteen distinct groups: betas with an exact 1 - beta in f32 (k / 16, 1 - 2^-k), learning rates between 2^-9 and 3e-3"""
    return [group(2.0 ** -9 * (1 + 0.03 * i), 0.5 + (i % 8) / 16.0, 1 - 2.0 ** -(5 + i % 6), 1e-8 * (1 + i), 0.01 * (i % 4), step=2 + i % 3)
            for i in range(16)]


def adamw_ref(p, g, m, v, h):
    """torch.optim.AdamW's single-tensor update (no amsgrad, no maximize) in fp64 from the hyper-parameters as the f32 struct `h`
    holds them, with decay = (float)(1.0 - (double)lr * (double)weight_decay) and step = (float)((double)lr / bias_corr1) formed as
    include/klab_mm.h states.  Returns (m', v', p'' - p)."""
    decay = f32(1.0 - h["lr"] * h["weight_decay"])
    step = f32(h["lr"] / h["bias_corr1"])
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    m = m + (1.0 - h["beta1"]) * (g - m)
    v = h["beta2"] * v + (1.0 - h["beta2"]) * g * g
    denom = v.sqrt() / (h["bias_corr2"] ** 0.5) + h["eps"]
    return m, v, (p * decay - step * (m / denom)) - p


def adamw_f32(p, g, m, v, h):
    """the same sequence with every operation rounded to f32 (no fused multiply-add): what a kernel that follows the header may
    return at worst.  Returns (m', v', p'')."""
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    decay, step = t(f32(1.0 - h["lr"] * h["weight_decay"])), t(f32(h["lr"] / h["bias_corr1"]))
    omb1, b2, omb2 = t(1.0) - t(h["beta1"]), t(h["beta2"]), t(1.0) - t(h["beta2"])
    inv = t(1.0) / torch.sqrt(t(h["bias_corr2"]))
    pd = p * decay
    m1 = m + omb1 * (g - m)
    v1 = b2 * v + (omb2 * g) * g
    denom = torch.sqrt(v1) * inv + t(h["eps"])
    return m1, v1, pd - step * (m1 / denom)


def errors(p0, p1, m1, v1, ref):
    """(m, v: worst relative error in units of 2^-24; dp: worst error as a fraction of its bound 1e-5 |dp_ref| + 3 2^-24 |p|)"""
    m_ref, v_ref, dp_ref = ref
    rm = float(((m1.double() - m_ref).abs() / m_ref.abs()).max()) / U24
    rv = float(((v1.double() - v_ref).abs() / v_ref.abs()).max()) / U24
    dp = p1.double() - p0.double()
    rp = float(((dp - dp_ref).abs() / (1e-5 * dp_ref.abs() + 3 * U24 * p0.double().abs())).max())
    return rm, rv, rp


M_V_ULPS = 4.0  # the bound of the existing Adam test on m and v


def draw(g, k):
    """k elements of the fixtures' distribution: magnitudes in [0.5, 2), random signs, m with the sign of g, v > 0"""
    mag = lambda: 0.5 + 1.5 * torch.rand(k, generator=g)
    sgn = lambda: torch.randint(0, 2, (k,), generator=g).float() * 2 - 1
    p, gr = mag() * sgn(), mag() * sgn()
    return p, gr, mag() * gr.sign(), mag() ** 2


class AdamWState:
    """n tensors as slices of flat buffers, the recipe of the Adam test: p (with gaps), grads / m / v at goff (another layout with
    gaps), compute-dtype copies at aoff in an arena (every third tensor has none: aoff = -1).  The arena starts as NaN; the gaps
    are ordinary values whose bits must survive.  group_of[i] = i % ngroups."""

    def __init__(self, n, seed, arena_dtype=torch.bfloat16):
        g = R.gen(seed)
        self.n = n
        self.lens = R.table_lengths(n, seed)
        self.poff, ptot = R.layout(self.lens, lambda i: 4 * (i % 2))
        self.goff, gtot = R.layout(self.lens, lambda i: 4 * ((i + 1) % 3))
        self.has_a = [i % 3 != 1 for i in range(n)]
        aoff, atot = R.layout([ln if h else 0 for ln, h in zip(self.lens, self.has_a)], lambda i: 4 * (i % 2))
        self.aoff = [a if h else -1 for a, h in zip(aoff, self.has_a)]
        self.pre, self.total4 = R.prefix4(self.lens)
        self.p = draw(g, ptot)[0]
        _p, self.g, self.m, self.v = draw(g, gtot)
        self.arena = torch.full((max(atot, 4),), float("nan"), dtype=arena_dtype)

    def groups_of(self, ngroups):
        return [i % ngroups for i in range(self.n)]

    def masks(self, tensors):
        """bool masks over p / the grads layout / the arena: the elements of the listed tensors"""
        mp, mg, ma = torch.zeros_like(self.p, dtype=torch.bool), torch.zeros_like(self.g, dtype=torch.bool), torch.zeros(len(self.arena), dtype=torch.bool)
        for i in tensors:
            mp[self.poff[i]:self.poff[i] + self.lens[i]] = True
            mg[self.goff[i]:self.goff[i] + self.lens[i]] = True
            if self.has_a[i]:
                ma[self.aoff[i]:self.aoff[i] + self.lens[i]] = True
        return mp, mg, ma

    def gather(self, flat, offs, tensors=None):
        tensors = range(self.n) if tensors is None else tensors
        return torch.cat([flat[offs[i]:offs[i] + self.lens[i]] for i in tensors])


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
