"""Store members of klab_gemm_grouped_tiles (accumulate = 0 per member): the product is written, C is never read.

Operands are the integers in [-3, 3] of tests/exact_ref.py, so every result is exact in f32 whatever the summation order and the
assertion is torch.equal with the fp64 product.  A store member's C starts as NaN inside [M, N]: a copy-out that still reads C, a
store member split along K (partial products overwriting each other, or atomics onto NaN) and a tile left unwritten all fail it.
C sits in a sentinel-filled buffer (ldc > N, a guard row before and after): every byte outside [M, N] must come back unchanged.
Accumulating members of the same list start from an integer C0 and must still add to it.

The shapes are the smallest that reach each form.  256 x 256 kernel (mm8p_grouped_try: M, N >= 128, K % 64 == 0, K >= 1024): one
tile ragged in M and in N; two tiles each way.  128-wide kernel (klab_gemm_grouped_tiles in gemm.hip): with so little work in the
list a workgroup's share is 16 k-tiles of 32, so an ACCUMULATING member of K = 2048 runs as (64 + 8) / 16 = 4 splits -- the store
members of that K must not; N < 128 anywhere in the list selects the 128 x 64 tiles.  A member that does not fit the grouped form
(M < 128) goes through klab_gemm, which stores without splitting as well."""
import math

import pytest
import torch

from tests import exact_ref as R
from tests.test_gemm_exact_gpu import Out, check_bound, operand

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
ALPHAS = (1.0, 0.5, -2.0)


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


class Member:
    """C [M, N] (=|+=) alpha * A B^T on the integer operands of (M, N, K); store: C starts as NaN, else as the integer C0"""

    def __init__(self, M, N, K, store, alpha=1.0, seed=0):
        self.M, self.N, self.K, self.store, self.alpha = M, N, K, store, alpha
        A, B, self.prod = R.gemm_ints(M, N, K, seed)
        self.Ad, self.Bd = operand(A, BF16, False), operand(B, BF16, False)
        self.c0 = None if store else R.gemm_extras(M, N, seed)["c0"]
        self.out = Out(M, N, torch.float32, c0=torch.full((M, N), math.nan) if store else self.c0)

    def args(self):
        return dict(A=self.Ad, B=self.Bd, C=self.out.C, M=self.M, N=self.N, K=self.K, a_kmajor=False, b_kmajor=False, ldc=self.out.ldc,
                    alpha=self.alpha, accumulate=not self.store, atomic_ok=True)

    def check(self, what):
        self.out.check(R.gemm_expected(self.prod, alpha=self.alpha, c0=self.c0),
                       f"{what}: {'store' if self.store else 'accumulate'} member ({self.M}, {self.N}, {self.K}) alpha {self.alpha}")


def run(ops, members, large, what):
    ops.gemm_grouped([m.args() for m in members], large_tiles=large)
    for m in members:
        m.check(what)


# (M, N, K): see the module docstring
LARGE_SHAPES = [(200, 136, 1024), (264, 264, 1088), (128, 128, 1024)]
WIDE_SHAPES = [(136, 136, 2048), (264, 200, 2048), (128, 128, 512)]
NARROW_SHAPES = [(136, 72, 2048), (128, 64, 512), (264, 136, 1024)]
LISTS = {"256x256": (LARGE_SHAPES, True), "128x128": (WIDE_SHAPES, False), "128x64": (NARROW_SHAPES, False)}


@pytest.mark.parametrize("name", list(LISTS))
def test_every_member_stores(ops, name):
    shapes, large = LISTS[name]
    run(ops, [Member(*s, store=True, alpha=ALPHAS[i % 3], seed=i) for i, s in enumerate(shapes)], large, name)


@pytest.mark.parametrize("name", list(LISTS))
def test_store_and_accumulate_members_in_one_launch(ops, name):
    # each shape twice: once storing onto NaN, once adding to C0 (on the 128-wide kernels the K = 2048 accumulating member is split)
    shapes, large = LISTS[name]
    members = []
    for i, s in enumerate(shapes):
        members.append(Member(*s, store=i % 2 == 0, alpha=ALPHAS[i % 3], seed=i))
        members.append(Member(*s, store=i % 2 == 1, alpha=ALPHAS[(i + 1) % 3], seed=10 + i))
    run(ops, members, large, f"mixed {name}")


def test_large_tile_list_with_one_unfit_member_falls_back_whole(ops):
    # K = 1056 is no multiple of 64: the whole list runs on the 128-wide kernel, where the store members (K = 2048 among them: four
    # splits if it accumulated) are not split
    shapes = [(200, 136, 2048, True), (256, 136, 1056, True), (264, 264, 1024, False), (128, 128, 2048, True)]
    run(ops, [Member(M, N, K, store=st, alpha=ALPHAS[i % 3], seed=i) for i, (M, N, K, st) in enumerate(shapes)], True, "fallback")


def test_store_member_that_goes_through_klab_gemm(ops):
    # M = 64 < 128 does not fit the grouped form: klab_gemm runs it between the grouped members, storing without split-K
    shapes = [(136, 136, 2048, True), (64, 128, 2048, True), (128, 128, 1024, False), (64, 136, 1024, False)]
    run(ops, [Member(M, N, K, store=st, alpha=ALPHAS[i % 3], seed=i) for i, (M, N, K, st) in enumerate(shapes)], False, "klab_gemm member")


@pytest.mark.parametrize("name,M,N,K,large", [("256x256", 264, 264, 1088, True), ("128x128", 264, 136, 2048, False),
                                              ("128x64", 136, 72, 2048, False)], ids=["256x256", "128x128", "128x64"])
def test_store_on_random_operands_per_element(ops, name, M, N, K, large):
    # randn operands, C = NaN before: every element within exact_ref.gemm_bound of the fp64 product
    A, B, ref, mag = R.gemm_randn(M, N, K)
    out = Out(M, N, torch.float32, c0=torch.full((M, N), math.nan))
    ops.gemm_grouped([dict(A=operand(A, BF16, False), B=operand(B, BF16, False), C=out.C, M=M, N=N, K=K, a_kmajor=False, b_kmajor=False,
                           ldc=out.ldc, accumulate=False, atomic_ok=True)], large_tiles=large)
    torch.cuda.synchronize()
    got = out.buf.cpu()
    check_bound(got[1:1 + M, :N], ref, R.gemm_bound(mag, K, ref), f"store {name}")
    got[1:1 + M, :N] = out.before[1:1 + M, :N]
    assert torch.equal(got.view(torch.int32), out.before.view(torch.int32))
