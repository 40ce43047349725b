"""Inputs and fp64 references for tests/test_engine_kernels_gpu.py: the entry points only the engine calls (grouped weight
gradients, deferred RMS-norm / position-bias gradients, the descriptor-table kernels).  Everything here is plain torch on the
CPU; the tests upload the operands and compare what the kernels leave behind."""
import numpy as np
import torch

U24 = 2.0 ** -24  # unit roundoff of f32


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, lo, hi, *shape, dtype=torch.float32):
    """integers drawn uniformly from lo .. hi (inclusive), stored in `dtype`"""
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


# ---- grouped GEMM ------------------------------------------------------------------------------------------------------------
C_SENTINEL = -12345.0


class Member:
    """One weight-gradient product C[M, N] += alpha * A^T B with A stored [K, lda] and B stored [K, ldb] (both m-major, bf16) and
    C [M, ldc] f32.  a_off > 0: A is the column block a_off .. a_off + M of a wider buffer (pointer offset a_off elements).
    The host copies are the truth; upload() makes the device buffers, args() the keywords for ops.gemm_grouped."""

    def __init__(self, g, M, N, K, alpha=1.0, lda=None, a_off=0, ldb=None, ldc=None, real=False):
        self.M, self.N, self.K, self.alpha = M, N, K, alpha
        self.lda = lda if lda is not None else M + a_off
        self.ldb, self.ldc, self.a_off = ldb or N, ldc or N, a_off
        assert self.lda >= a_off + M and self.ldb >= N and self.ldc >= N and a_off % 8 == 0
        if real:
            self.Abuf = torch.randn(K, self.lda, generator=g).bfloat16()
            self.Bbuf = torch.randn(K, self.ldb, generator=g).bfloat16()
            c0 = torch.randn(M, N, generator=g)
        else:
            self.Abuf = ints(g, -4, 4, K, self.lda, dtype=torch.bfloat16)
            self.Bbuf = ints(g, -4, 4, K, self.ldb, dtype=torch.bfloat16)
            c0 = ints(g, -8, 8, M, N)
        self.C0 = torch.full((M, self.ldc), C_SENTINEL)
        self.C0[:, :N] = c0

    @property
    def A(self):
        return self.Abuf[:, self.a_off:self.a_off + self.M]

    @property
    def B(self):
        return self.Bbuf[:, :self.N]

    def upload(self):
        self.Ad, self.Bd, self.Cd = self.Abuf.cuda(), self.Bbuf.cuda(), self.C0.cuda()
        return self

    def args(self):
        return dict(A=self.Ad[:, self.a_off:], B=self.Bd, C=self.Cd, M=self.M, N=self.N, K=self.K, a_kmajor=False, b_kmajor=False,
                    lda=self.lda, ldb=self.ldb, ldc=self.ldc, alpha=self.alpha, accumulate=True, atomic_ok=True)

    def product(self):
        return self.A.double().T @ self.B.double()

    def expected(self):
        """C0 + alpha * A^T B in fp64 (exact for the integer operands), with the sentinel columns of the C buffer kept"""
        want = self.C0.double()
        want[:, :self.N] += self.alpha * self.product()
        return want

    def bound(self):
        """per-element worst case of K f32 additions of exact products, doubled for faithful (not round-to-nearest) adds in the
        matrix unit: 2 (K + 2) 2^-24 (sum_k |a| |b| + |C0|)"""
        mag = self.A.double().abs().T @ self.B.double().abs() + self.C0[:, :self.N].double().abs()
        return 2.0 * (self.K + 2) * U24 * mag


# ---- descriptor tables -------------------------------------------------------------------------------------------------------
def table_lengths(n, seed):
    """element counts (multiples of 4) of n tensors: from one vec4 to a few thousand elements, most of them shorter than 256
    vec4, so that one thread's unrolled batch of vec4's (a block width apart) walks across many descriptors"""
    g = gen(seed)
    n4 = torch.randint(1, 65, (n,), generator=g)
    n4[::7] = torch.randint(256, 1200, (len(n4[::7]),), generator=g)
    n4[0], n4[-1] = 1, 1
    if n >= 3:
        n4[1] = 750
    return [int(v) * 4 for v in n4]


def layout(lengths, gap_of, align=4):
    """offsets of tensors laid out one after the other with a gap of gap_of(i) elements behind tensor i -> (offsets, total)"""
    offs, pos = [], 0
    for i, n in enumerate(lengths):
        offs.append(pos)
        pos += n + gap_of(i)
        pos = (pos + align - 1) // align * align
    return offs, pos


def prefix4(lengths):
    """exclusive prefix sums of the lengths in vec4 units, and their total"""
    p = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64) // 4)])
    return [int(v) for v in p[:-1]], int(p[-1])


def with_bf16_ties(x, g, every=5):
    """every `every`-th element of the f32 tensor x replaced by a value exactly half way between two neighbouring bf16 values
    (the low 16 bits 0x8000), the bf16 below it having an even or an odd last bit as the random source value had"""
    bits = x.contiguous().view(torch.int32).clone()
    flat = bits.view(-1)
    flat[::every] = (flat[::every] & -65536) | 0x8000
    return flat.view(torch.float32).view(x.shape)


def adam_ref(p, g, m, v, lr, beta1, beta2, eps, wd, bc1, bc2):
    """torch.optim.Adam's single-tensor update (no amsgrad, L2 weight decay) in fp64, from the hyper-parameters as f32 holds them"""
    f = lambda a: float(np.float32(a))
    lr, beta1, beta2, eps, wd, bc1, bc2 = map(f, (lr, beta1, beta2, eps, wd, bc1, bc2))
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    g = g + wd * p
    m = m + (1.0 - beta1) * (g - m)
    v = beta2 * v + (1.0 - beta2) * g * g
    denom = v.sqrt() / (bc2 ** 0.5) + eps
    return m, v, -(lr / bc1) * (m / denom)
