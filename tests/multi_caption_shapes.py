"""Shapes of the kernel-level tests of grouped cross-attention (tests/test_multi_caption_attn_gpu.py), shared with the CPU test that
proves their fixtures exact (tests/test_multi_caption_cpu.py).

The engine issues the cross-attention of an image's n captions as ONE batch element with Lq = n*Lt queries over the image's Lk = Le
keys.  (Lq, n): 15 = 3 x 5 sits inside one 16-query tile of every kernel; 85 = 5 x 17 crosses the 64-query tile of the matrix-core
kernels and is ragged in both tile sizes; 64 = 2 x 32 fills one exactly.  Lk = 65 is one key past a 64-key block, 80 is no multiple
of 32.  Two images with different operands, six heads (T5-small's 8 would add nothing a sixth head does not), head dim 64 (the
headline model's) and, at the ragged shape, 32."""
from tests import exact_ref as R

XATTN_B, XATTN_H = 2, 6
# (Lq, n, Lk, dk)
XATTN_SHAPES = [(15, 3, 65, 64), (15, 3, 80, 64), (85, 5, 65, 64), (85, 5, 80, 64), (64, 2, 65, 64), (64, 2, 80, 64), (85, 5, 65, 32)]


def xattn_kinds(dk):
    """the dyadic fixtures of exact_ref at this head dim, and the one whose one-hot rows come from the scores alone: T5
    cross-attention has no position bias, and that is the form the engine calls"""
    return R.fixtures_for(dk) + (("onehot_nobias", 1),)


def caption_slices(Lq, n):
    Lt = Lq // n
    assert Lt * n == Lq
    return [slice(j * Lt, (j + 1) * Lt) for j in range(n)]
