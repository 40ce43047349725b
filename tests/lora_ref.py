"""fp64 statements of the two LoRA kernels (csrc/lora.hip), their per-element bounds and the fixtures, shared by
tests/test_lora_cpu.py (which proves the bounds on three f32 evaluation orders and the exactness of the integer fixtures) and the
GPU tests.  Plain torch on the CPU.

For a target W [out, in] with A [r, in], B [out, r] and the scalar s:

    merge   exact = W + s B A                      |got - exact| <= gamma(r + 2) (|W| + |s| |B| |A|) + half a spacing of the arena type at exact
    dB      exact = s dW A^T                       |got - exact| <= gamma(in + 1)  |s| |dW| |A|^T
    dA      exact = s B^T dW                       |got - exact| <= gamma(out + 1) |s| |B|^T |dW|

with u = 2^-24 and gamma(n) = n u / (1 - n u): standard f32 summation of n terms in any order (each term passes through at most n
roundings: its product, the additions above it, the scale), with or without fused multiply-adds.  2^-149 covers a result in the
denormal range."""
import torch

U24 = 2.0 ** -24
SHAPES = ((64, 64), (136, 200), (520, 72))  # multiples of 4, not of the 64 x 64 tile; 136 and 520 rows end in a partial row block
RANKS = (1, 3, 8, 16, 64)
NTAB = (1, 7)
S_INT = 0.5  # the integer fixtures' scale: a power of two
S_RND = 2.0


def gamma(n):
    return n * U24 / (1.0 - n * U24)


def half_spacing(x, dtype):
    """half the spacing of `dtype` (torch.bfloat16 or torch.float32) at the fp64 values x"""
    _m, e = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))  # |x| = m 2^e, 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - (9 if dtype == torch.bfloat16 else 25))


def merge_ref(W, A, B, s, dtype):
    """(exact, bound) of the merge into an arena of `dtype`"""
    exact = W.double() + s * (B.double() @ A.double())
    mag = W.double().abs() + abs(s) * (B.double().abs() @ A.double().abs())
    return exact, gamma(A.shape[0] + 2) * mag + half_spacing(exact, dtype) + 2.0 ** -149


def grads_ref(dW, A, B, s):
    """(dA, bound of dA, dB, bound of dB)"""
    d, a, b = dW.double(), A.double(), B.double()
    dA, dB = s * (b.t() @ d), s * (d @ a.t())
    return (dA, gamma(dW.shape[0] + 1) * abs(s) * (b.abs().t() @ d.abs()) + 2.0 ** -149,
            dB, gamma(dW.shape[1] + 1) * abs(s) * (d.abs() @ a.abs().t()) + 2.0 ** -149)


def worst(got, exact, bound):
    """the worst error of `got` as a fraction of its bound"""
    return float(((got.double() - exact).abs() / bound).max())


def must_move(W, A, B, s, dtype):
    """elements the merge has to change: |s (B A)[i,j]| exceeds one spacing of the arena type at W[i,j]"""
    return (s * (B.double() @ A.double())).abs() > 2.0 * half_spacing(W, dtype)


# ---- three f32 evaluation orders -----------------------------------------------------------------------------------------------------
def _sum_f32(terms, order):
    """the f32 sum of a list of f32 tensors, every addition rounded to f32"""
    if order == "forward" or order == "reverse":
        seq = terms if order == "forward" else terms[::-1]
        acc = seq[0].clone()
        for t in seq[1:]:
            acc = acc + t
        return acc
    assert order == "pairwise"
    while len(terms) > 1:
        terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
    return terms[0]


ORDERS = ("forward", "reverse", "pairwise")


def merge_f32(W, A, B, s, order, dtype):
    """every product and every addition rounded to f32 (no fused multiply-add), the rank sum in `order`, one cast into `dtype`"""
    acc = _sum_f32([B[:, k, None] * A[None, k, :] for k in range(A.shape[0])], order)
    return (W + torch.tensor(s, dtype=torch.float32) * acc).to(dtype)


def grads_f32(dW, A, B, s, order):
    s = torch.tensor(s, dtype=torch.float32)
    dA = s * _sum_f32([B[i, :, None] * dW[None, i, :] for i in range(dW.shape[0])], order)
    dB = s * _sum_f32([dW[:, j, None] * A[None, :, j] for j in range(dW.shape[1])], order)
    return dA, dB


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------
GAP = 16  # sentinel elements around every tensor of the arena, the gradient buffer, the outputs and the slab


class Fixture:
    """n target tensors of mixed shapes with rank r.  kind "int": small integers and s = 1/2 (every product and every partial sum is
    exact in f32 in any order, the merged value fits 8 bits); kind "randn": W ~ 0.02 N(0, 1), A, B, dW ~ N(0, 1), s = 2 (s B A is far
    above the arena's spacing at W almost everywhere).  b_zero: B = 0.
    Layouts: arena tensor i at aoff[i], dW of tensor i at goff[i], GAP sentinel elements between neighbours, and one arena tensor
    (`other`) that is in no table."""

    def __init__(self, n, r, kind, seed=0, b_zero=False):
        g = torch.Generator().manual_seed(1000 * seed + 10 * r + n)
        self.n, self.r, self.kind = n, r, kind
        self.s = S_INT if kind == "int" else S_RND
        self.shapes = [SHAPES[1]] if n == 1 else [SHAPES[(i * 2 + i // 3) % 3] for i in range(n)]
        ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).float()
        rn = lambda shape: torch.randn(shape, generator=g)
        self.W, self.A, self.B, self.dW = [], [], [], []
        for o, i in self.shapes:
            if kind == "int":
                self.W.append(ri(-8, 8, (o, i))); self.A.append(ri(-1, 1, (r, i))); self.B.append(ri(-1, 1, (o, r)))
                self.dW.append(ri(-4, 4, (o, i)))
            else:
                self.W.append(0.02 * rn((o, i))); self.A.append(rn((r, i))); self.B.append(rn((o, r))); self.dW.append(rn((o, i)))
            if b_zero:
                self.B[-1].zero_()
        self.aoff, self.goff = [], []
        run = GAP
        for o, i in self.shapes:
            self.aoff.append(run)
            run += o * i + GAP
        self.other = run  # an arena tensor of 256 elements that no table entry names
        self.arena_elems = run + 256 + GAP
        run = GAP
        for o, i in reversed(self.shapes):  # (the gradient layout follows the backward order: another order than the arena's)
            self.goff.insert(0, run)
            run += o * i + GAP
        self.grad_elems = run

    def arena(self, dtype):
        """the arena before the merge: a sentinel pattern no result equals"""
        return torch.full((self.arena_elems,), -7.75, dtype=dtype)

    def grads(self):
        flat = torch.full((self.grad_elems,), 3.0e38)
        for d, go in zip(self.dW, self.goff):
            flat[go:go + d.numel()] = d.reshape(-1)
        return flat

    def arena_mask(self):
        m = torch.zeros(self.arena_elems, dtype=torch.bool)
        for (o, i), ao in zip(self.shapes, self.aoff):
            m[ao:ao + o * i] = True
        return m
