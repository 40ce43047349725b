"""The kernels of csrc/adafactor.hip on the shapes real T5 weights have and on every limit of the tile plan, through the raw entry
point: each instantiation of the tile walk (16-byte and scalar columns; 1, 2, 4 and 8 column steps, the last one partly
filled), rows that span 2 and 4 waves, tall tensors (tile length by count, the 512-row cap, more than 8 and a non-multiple of
8 column partials), a 1-D tensor of several tiles, and more tiles than the grid has workgroups.

Reference: tests/adafactor_ref.py in float64.  Yardstick: the per-parameter torch rule of optim.py in fp32 on the same inputs.
Parameters follow the 2x rule of tests/test_adafactor_gpu.py (iii): distance to float64, in units of the displacement, at most
twice the torch rule's.  States (R, C, V, first moment; relative to their own norm) follow the same rule with a floor of one
fp32 rounding, 2^-23, under the yardstick: a vector of eight row means, each a sum of 8192 terms taken in another order, can
sit closer to float64 than one rounding by luck on either side, and no fp32 code can be held to twice that."""
import numpy as np
import pytest
import torch

from tests import adafactor_ref as R
from tests.test_adafactor_gpu import Raw

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
STEPS = 3
SETTINGS = {"default": {}, "momentum_decay": dict(beta1=0.9, weight_decay=0.01)}
# shape -> what it exercises
LIMITS = [
    (96, 512),     # 2 waves per row, two rows per sweep (every d_model-wide weight of t5-small)
    (40, 1024),    # 4 waves per row
    (40, 2048),    # 2 column steps (wo.weight of t5-small is 512 x 2048)
    (36, 1028),    # 2 column steps, the second one 4 columns wide
    (24, 4096),    # 4 column steps (d_ff of t5-large)
    (12, 2816),    # 4 column steps, the last partly filled (d_ff of t5-v1_1-large)
    (8, 8192),     # 8 column steps: the stated limit
    (16, 517),     # scalar columns, 8 column steps (3 used)
    (32, 6),       # scalar columns, 128 rows per sweep (relative_attention_bias with 6 heads)
    (384, 512), (512, 384),  # q / o of t5-v1_1-small: 96 of 128 lanes on a row
    (70000, 64),   # tile length from the 512-row cap: 137 tiles, column partials 17 x 8 + 1
    (40000, 512),  # tile length by count (316 rows): 127 tiles of a shared.weight-like table
    (40000,),      # 1-D, three tiles
    (512,),        # a norm weight
]
MANY = [(2048, 512)] * 36 + [(512,)] * 4  # 36 x 64 tiles + 4 > 2048 workgroups: the grid-stride loop


def make_inputs(shapes, seed):
    rng = np.random.default_rng(seed)
    p0 = [(rng.standard_normal(s) * 0.05).astype(np.float32) for s in shapes]
    grads = []
    for t in range(STEPS):
        gs = []
        for s in shapes:
            g = (rng.standard_normal(s) * 10.0 ** rng.uniform(-3, -1)).astype(np.float32)
            if len(s) == 2:
                g[::3] = 0.0  # rows no token hit
            gs.append(g)
        grads.append(gs)
    return p0, grads


def torch_rule(p0, grads, kw):
    from klab_multimodalmodel_amd.optim import FusedAdafactor
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy()).cuda()) for p in p0]
    opt = FusedAdafactor(ps, **kw)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g).cuda()
        opt.step()
    assert opt._fb_reason is not None and not opt._flat_live
    return ps, opt


def check(shapes, seed, kw):
    p0, grads = make_inputs(shapes, seed)
    runs = []
    for _ in range(2):
        raw = Raw(kw, shapes=shapes, p0=p0)
        for gs in grads:
            raw.step(gs)
        torch.cuda.synchronize()
        runs.append(raw)
    a, b = runs
    for x, y in zip(a.p + [a.state, a.scal] + ([a.m] if a.m is not None else []), b.p + [b.state, b.scal] + ([b.m] if b.m is not None else [])):
        assert torch.equal(x, y)  # bit-reproducible
    ps, opt = torch_rule(p0, grads, kw)
    ref_p, ref_st = R.run_f64(p0, grads, **kw)
    fails, worst = [], 0.0
    for i, s in enumerate(shapes):
        assert torch.isfinite(a.p[i]).all()
        e, y = R.displacement_err(a.p[i].cpu().numpy(), ref_p[i], p0[i]), R.displacement_err(ps[i].detach().cpu().numpy(), ref_p[i], p0[i])
        worst = max(worst, e / y)
        if not e <= 2 * y:
            fails.append((i, s, "p", e, y))
        if len(s) == 2:
            assert torch.equal(a.arena[a.goff[i]:a.goff[i] + a.p[i].numel()].view_as(a.p[i]), a.p[i])
        for k, v in a.states(i).items():
            assert torch.isfinite(v).all()
            e, y = R.rel_err(v.cpu().numpy(), ref_st[i][k]), R.rel_err(opt.state[ps[i]][k].cpu().numpy(), ref_st[i][k])
            if not e <= 2 * max(y, EPS32):
                fails.append((i, s, k, e, y))
        rms = float(a.scal[4 * i + 1])
        assert abs(rms - ref_st[i]["RMS"]) <= 1e-5 * rms
    print(f"{len(shapes)} tensors: worst parameter error / torch rule's = {worst:.3f}")
    assert not fails, fails


@pytest.mark.parametrize("name", list(SETTINGS))
def test_every_tile_walk_and_plan_limit(name):
    check(LIMITS, 11, SETTINGS[name])


def test_more_tiles_than_workgroups():
    check(MANY, 12, SETTINGS["momentum_decay"])


def test_plan_of_these_shapes():
    """the shapes above really land where the comments say (tile length, tile count)"""
    import ctypes as C

    from klab_multimodalmodel_amd import _lib as L
    lib = L.load()
    want = {(70000, 64): (512, 137), (40000, 512): (316, 127), (2048, 512): (32, 64), (96, 512): (32, 3), (8, 8192): (4, 2)}
    for s, (tl, ntl) in want.items():
        rows, cols, fact = (C.c_long * 1)(s[0]), (C.c_long * 1)(s[1]), (C.c_int * 1)(1)
        out, tot = (C.c_long * 4)(), (C.c_long * 4)()
        assert lib.klab_adafactor_plan(1, rows, cols, fact, out, tot) == 0
        assert (out[2], tot[1]) == (tl, ntl), (s, out[2], tot[1])
    n = len(MANY)
    rows = (C.c_long * n)(*[s[0] if len(s) == 2 else 1 for s in MANY])
    cols = (C.c_long * n)(*[s[-1] for s in MANY])
    fact = (C.c_int * n)(*[len(s) == 2 for s in MANY])
    out, tot = (C.c_long * (4 * n))(), (C.c_long * 4)()
    assert lib.klab_adafactor_plan(n, rows, cols, fact, out, tot) == 0 and tot[1] > 2048
