"""Reference tests for the entry points only engine.cpp calls: klab_gemm_grouped[_tiles] (the 128-wide split-K kernel and the
256 x 256 kernel behind it), the deferred RMS-norm weight gradient (klab_rmsnorm_bwd_part + klab_colpart_reduce), the deferred
position-bias gradient (ds_defer + klab_dbias_reduce), the three descriptor-table kernels (klab_cast_pack, klab_quant_fp8_arena,
klab_adam_step[_range]) with their table in LDS and in global memory, and klab_ce_count.

Where the arithmetic allows it the inputs are chosen so that the result is EXACT in f32 whatever the summation order (small
integers), and the assertion is torch.equal: one wrong row, a ragged edge tile dropped or added twice, a group member picked by
an off-by-one start all fail it.  The remaining bounds are per element and derived from the f32 format, not measured."""
import numpy as np
import pytest
import torch

from tests import engine_kernels_ref as R
from tests.engine_kernels_ref import Member, U24

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


def seed_word(v=1234):
    return torch.tensor([v], dtype=torch.int32).cuda()


# ---------------------------------------------------------------------------------------------------------------- grouped GEMM
ALPHAS = (1.0, 0.5, -2.0)


def run_group(ops, members, large_tiles):
    for m in members:
        m.upload()
    ops.gemm_grouped([m.args() for m in members], large_tiles=large_tiles)
    torch.cuda.synchronize()
    return [m.Cd.cpu() for m in members]


def assert_exact(members, got):
    for i, (m, c) in enumerate(zip(members, got)):
        want = m.expected()
        bad = (c.double() != want)
        assert not bool(bad.any()), (f"member {i} (M, N, K) = ({m.M}, {m.N}, {m.K}): {int(bad.sum())} wrong elements, rows "
                                     f"{bad.any(1).nonzero().flatten()[:8].tolist()} cols {bad.any(0).nonzero().flatten()[:8].tolist()}")
        assert torch.equal(c.double(), want)


# (M, N, K) and the strides: lda > M as a column block at an offset, ldb > N, ldc > N at least once per list
NARROW = [dict(M=128, N=64, K=512), dict(M=136, N=72, K=544, lda=136 + 24 + 16, a_off=24), dict(M=384, N=200, K=2048, ldb=208, ldc=204),
          dict(M=264, N=64, K=1024, ldc=72), dict(M=128, N=128, K=4096, lda=128 + 8, a_off=8, ldb=136), dict(M=128, N=64, K=8192)]
WIDE = [dict(M=128, N=128, K=512, ldc=132), dict(M=520, N=136, K=1536, lda=520 + 64 + 8, a_off=64, ldb=144), dict(M=256, N=384, K=2048, ldc=392)]


@pytest.mark.parametrize("shapes", [NARROW, WIDE], ids=["narrow_bn64", "wide_bn128"])
def test_grouped_split_k_kernel_is_exact_on_integers(ops, shapes):
    g = R.gen(11)
    members = [Member(g, alpha=ALPHAS[i % 3], **s) for i, s in enumerate(shapes)]
    assert_exact(members, run_group(ops, members, large_tiles=False))


def test_grouped_two_launches_with_members_that_go_through_klab_gemm(ops):
    # eleven fitting members: launches of 8 + 3, `start` restarts at 0 for the second; K = 520 (no multiple of 32) and M = 64 do not
    # fit and run through klab_gemm between them
    g = R.gen(12)
    fit = [dict(M=128, N=64, K=512), dict(M=136, N=72, K=544, ldc=80), dict(M=128, N=128, K=1024), dict(M=264, N=64, K=512, ldb=72),
           dict(M=128, N=64, K=2048), dict(M=144, N=136, K=512, lda=160, a_off=16), dict(M=128, N=72, K=1024), dict(M=256, N=64, K=512),
           dict(M=136, N=64, K=1536, ldc=68), dict(M=128, N=200, K=512), dict(M=272, N=64, K=544)]
    shapes = fit[:3] + [dict(M=128, N=64, K=520)] + fit[3:9] + [dict(M=64, N=128, K=512, ldc=136)] + fit[9:]
    assert len(shapes) == 13
    members = [Member(g, alpha=ALPHAS[i % 3], **s) for i, s in enumerate(shapes)]
    assert_exact(members, run_group(ops, members, large_tiles=False))


LARGE = [dict(M=136, N=264, K=1024), dict(M=256, N=256, K=1088, ldc=260), dict(M=520, N=128, K=1024, lda=520 + 8 + 8, a_off=8, ldb=136),
         dict(M=264, N=520, K=2048)]


def test_grouped_large_tile_kernel_is_exact_on_integers(ops):
    # ragged M and N edges, 1x2, 1x1, 3x1 and 2x3 tile grids, K = 1088: an odd number of 64-wide k-tiles
    g = R.gen(13)
    members = [Member(g, alpha=ALPHAS[i % 3], **s) for i, s in enumerate(LARGE)]
    assert_exact(members, run_group(ops, members, large_tiles=True))


@pytest.mark.parametrize("n", [32, 33], ids=["full_table", "one_too_many_falls_back"])
def test_grouped_large_tile_table_of_32_and_fallback_above(ops, n):
    g = R.gen(14)
    members = [Member(g, 128, 128, 1024, alpha=ALPHAS[i % 3]) for i in range(n)]
    assert_exact(members, run_group(ops, members, large_tiles=True))


def test_grouped_large_tile_list_with_one_unfit_member_falls_back_whole(ops):
    # K = 1056 is legal for the 128-wide kernel (a multiple of 32), not for the 256 x 256 one (no multiple of 64)
    g = R.gen(15)
    shapes = [dict(M=136, N=264, K=1024), dict(M=256, N=136, K=1056, ldc=140), dict(M=128, N=128, K=2048), dict(M=264, N=128, K=1024)]
    members = [Member(g, alpha=ALPHAS[i % 3], **s) for i, s in enumerate(shapes)]
    assert_exact(members, run_group(ops, members, large_tiles=True))


@pytest.mark.parametrize("shapes,large", [([dict(M=136, N=72, K=2048, ldc=80), dict(M=128, N=64, K=2048)], False),
                                          ([dict(M=264, N=136, K=2048, ldb=144), dict(M=128, N=128, K=2048)], False),
                                          ([dict(M=264, N=264, K=2048, ldc=268), dict(M=128, N=136, K=2048)], True)],
                         ids=["bn64", "bn128", "256x256"])
def test_grouped_kernels_on_realistic_data_per_element(ops, shapes, large):
    # randn operands: every element within the worst-case bound of K f32 additions of exact bf16 products (Member.bound); a
    # structure error (a k-tile dropped or doubled) is of order sqrt(32) here, the bound of order 1e-2
    g = R.gen(16)
    members = [Member(g, real=True, **s) for s in shapes]
    got = run_group(ops, members, large_tiles=large)
    for m, c in zip(members, got):
        want = m.expected()
        err = (c.double() - want)[:, :m.N].abs()
        ratio = float((err / m.bound()).max())
        print(f"grouped real ({m.M}, {m.N}, {m.K}) large={large}: max |err| {float(err.max()):.3e}, max err / bound {ratio:.3e}")
        assert ratio <= 1.0
        assert torch.equal(c[:, m.N:], m.C0[:, m.N:])


# ---------------------------------------------------------------------------------------- deferred RMS-norm weight gradient
def _rms_inputs(rows, d, variant, seed):
    g = R.gen(seed)
    x = torch.randn(rows, d, generator=g) * 2.0
    w = 1 + 0.1 * torch.randn(d, generator=g)
    dres = torch.randn(rows, d, generator=g)
    rstd = torch.rsqrt(x.pow(2).mean(1) + 1e-6)
    kw = {}
    yrows = rows
    ymap = torch.arange(rows)
    if variant == "remap":  # dy lives in a row space where every `grp` rows sit `off` rows into a block of grp_stride rows
        grp = rows // 3
        assert grp * 3 == rows
        kw = dict(grp=grp, grp_stride=grp + 20, off=7)
        yrows = 3 * (grp + 20)
        ymap = (ymap // grp) * (grp + 20) + ymap % grp + 7
    dy = torch.randn(yrows, d, generator=g)
    if variant == "drop":
        kw = dict(p_y=0.1, tag_y=5, p_prev=0.25, tag_prev=9, seed=seed_word(77))
    return x, w, dres, rstd, dy, kw, ymap


def _drop_mult(ops, rows, d, p, tag, seed):
    """the kernels' dropout multiplier of (seed, tag) at every element index of a [rows, d] matrix: rmsnorm_bwd's row kernel with
    dy = 0 and dres = 1 writes exactly 1 * multiplier to dxt"""
    one = torch.ones(rows, d, device="cuda")
    out = torch.empty(rows, d, device="cuda")
    ops.rmsnorm_bwd(torch.zeros(rows, d, device="cuda"), one, torch.ones(d, device="cuda"), torch.ones(rows, device="cuda"), dres=one, dxt=out,
                    p_prev=p, tag_prev=tag, seed=seed)
    return out.cpu()


def _dw_terms(ops, x, rstd, dy, kw, ymap):
    """fp64 per-row terms of the weight gradient as the kernel forms them: (dy * dropmask_y, rounded to f32) * x * rstd"""
    e = dy[ymap]
    if kw.get("p_y", 0.0) > 0:
        mult = _drop_mult(ops, dy.shape[0], dy.shape[1], kw["p_y"], kw["tag_y"], kw["seed"])
        assert 0.85 < float((mult != 0).float().mean()) < 0.95
        e = e * mult[ymap]  # one f32 multiply, as in the kernel
    return e.double() * x.double() * rstd.double()[:, None]


RMS_CASES = [(21, 128, ""), (300, 512, ""), (100, 132, ""), (70, 768, ""), (8200, 256, ""), (300, 512, "remap"), (100, 132, "drop"),
             (8200, 256, "drop")]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("rows,d,variant", RMS_CASES)
def test_rmsnorm_bwd_part_matches_rmsnorm_bwd_and_fp64_column_sums(ops, dt, rows, d, variant):
    x, w, dres, rstd, dy, kw, ymap = _rms_inputs(rows, d, variant, seed=21)
    xd, wd, dresd, rstdd, dyd = x.cuda(), w.cuda(), dres.cuda(), rstd.cuda(), dy.cuda()
    # the atomics form
    dx0, dxt0 = torch.empty(rows, d, device="cuda"), torch.empty(rows, d, device="cuda", dtype=dt)
    dw0 = torch.zeros(d, device="cuda")
    ops.rmsnorm_bwd(dyd, xd, wd, rstdd, dres=dresd, dx=dx0, dxt=dxt0, dw=dw0, **kw)
    # the deferred form: the same kernel with one flag
    pr = ops.rmsnorm_part_rows(rows)
    assert pr == min((rows + 15) // 16, 512)
    dx1, dxt1 = torch.empty(rows, d, device="cuda"), torch.empty(rows, d, device="cuda", dtype=dt)
    part = torch.full((pr + 1, d), float("nan"), device="cuda")
    ops.rmsnorm_bwd_part(dyd, xd, wd, rstdd, part, dres=dresd, dx=dx1, dxt=dxt1, **kw)
    torch.cuda.synchronize()
    assert torch.equal(dx1, dx0) and torch.equal(dxt1, dxt0)
    part = part.cpu()
    assert not bool(part[:pr].isnan().any())  # overwritten, not added to
    assert bool(part[pr].isnan().all())       # and nothing behind the last workgroup's row
    term = _dw_terms(ops, x, rstd, dy, kw, ymap)
    want, bound = term.sum(0), 2.0 * rows * U24 * term.abs().sum(0)
    got = part[:pr].double().sum(0)
    r_ref = float(((got - want).abs() / bound).max())
    r_atomic = float(((got - dw0.cpu().double()).abs() / bound).max())
    print(f"rmsnorm_bwd_part ({rows}, {d}) {variant}: err / bound vs fp64 {r_ref:.3e}, vs the atomics form {r_atomic:.3e}")
    assert r_ref <= 1.0
    assert r_atomic <= 1.0


@pytest.mark.parametrize("d", [132, 512])
@pytest.mark.parametrize("nparts", [1, 5, 512])
def test_colpart_reduce_is_exact_on_integers(ops, nparts, d):
    g = R.gen(31)
    ncalls, stride = 3, nparts * d + 40
    part = torch.full((ncalls * stride,), float("nan"))
    for c in range(ncalls):
        part[c * stride:c * stride + nparts * d] = R.ints(g, -8, 8, nparts * d)
    dst0 = R.ints(g, 1, 9, ncalls + 1, d)  # non-zero: the kernel adds; row 1 is not listed
    listed = [0, 2, 3]
    dst = dst0.cuda()
    ops.colpart_reduce(part.cuda(), stride, nparts, d, [dst[i] for i in listed])
    torch.cuda.synchronize()
    want = dst0.double()
    for c, i in enumerate(listed):
        want[i] += part[c * stride:c * stride + nparts * d].view(nparts, d).double().sum(0)
    assert torch.equal(dst.cpu().double(), want)


@pytest.mark.parametrize("rows,d", [(300, 512), (100, 132)])
def test_three_deferred_rmsnorm_calls_and_one_reduce(ops, rows, d):
    pr = ops.rmsnorm_part_rows(rows)
    stride = pr * d + 64
    part = torch.full((3 * stride,), float("nan"), device="cuda")
    dws = torch.zeros(3, d, device="cuda")
    ref_dw, bounds = [], []
    for c in range(3):
        x, w, dres, rstd, dy, kw, ymap = _rms_inputs(rows, d, "", seed=40 + c)
        dx = torch.empty(rows, d, device="cuda")
        ops.rmsnorm_bwd_part(dy.cuda(), x.cuda(), w.cuda(), rstd.cuda(), part[c * stride:], dres=dres.cuda(), dx=dx)
        dw = torch.zeros(d, device="cuda")
        ops.rmsnorm_bwd(dy.cuda(), x.cuda(), w.cuda(), rstd.cuda(), dres=dres.cuda(), dx=dx, dw=dw)
        ref_dw.append(dw.cpu().double())
        bounds.append(2.0 * rows * U24 * _dw_terms(ops, x, rstd, dy, kw, ymap).abs().sum(0))
    ops.colpart_reduce(part, stride, pr, d, [dws[c] for c in range(3)])
    torch.cuda.synchronize()
    for c in range(3):
        ratio = float(((dws[c].cpu().double() - ref_dw[c]).abs() / bounds[c]).max())
        print(f"deferred rmsnorm dw, call {c} of ({rows}, {d}): err / bound vs the atomics form {ratio:.3e}")
        assert ratio <= 1.0


# ---------------------------------------------------------------------------------------- deferred position-bias gradient
@pytest.mark.parametrize("B,H,Lq,Lk,dk", [(3, 2, 20, 20, 32), (2, 4, 7, 7, 16)])
def test_attention_bwd_ds_defer_then_dbias_reduce_equals_the_direct_form(ops, B, H, Lq, Lk, dk):
    g = R.gen(51)
    dt, inner, Lkp = torch.bfloat16, H * dk, (Lk + 31) // 32 * 32
    q, k, v = [(torch.randn(B * L, inner, generator=g) * 0.5).to(dt).cuda() for L in (Lq, Lk, Lk)]
    bias = torch.randn(H, Lq, Lk, generator=g).cuda()
    dctx = torch.randn(B * Lq, inner, generator=g).to(dt).cuda()
    ctx, lse = torch.zeros(B * Lq, inner, device="cuda", dtype=dt), torch.empty(B, H, Lq, device="cuda")
    kw = dict(B=B, H=H, Lq=Lq, Lk=Lk, dk=dk, bias=bias, causal=True)
    ops.t5_attn_fwd(q, k, v, ctx, lse, **kw)
    dbias0 = torch.randn(H, Lq, Lk, generator=g)
    outs = []
    for defer in (False, True):
        grads = [torch.zeros(B * L, inner, device="cuda", dtype=dt) for L in (Lq, Lk, Lk)]
        ws = torch.full((B * H * Lq * Lkp,), float("nan"), device="cuda", dtype=dt)
        dbias = dbias0.cuda()
        ops.t5_attn_bwd(q, k, v, ctx, lse, dctx, *grads, dbias=dbias, ds_ws=ws, ds_defer=defer, **kw)
        torch.cuda.synchronize()
        if defer:
            assert torch.equal(dbias.cpu(), dbias0)  # only dS was stored
            ops.dbias_reduce(ws, dbias, nbatch=B, H=H, Lq=Lq, Lk=Lk)
            torch.cuda.synchronize()
        outs.append([t.cpu() for t in grads] + [dbias.cpu()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not bool(outs[1][3].isnan().any()) and not torch.equal(outs[1][3], dbias0)


@pytest.mark.parametrize("H,Lq,Lk", [(2, 20, 20), (8, 64, 64)])
@pytest.mark.parametrize("nbatch", [1, 64, 65, 6 * 64])
def test_dbias_reduce_is_exact_on_integers(ops, nbatch, H, Lq, Lk):
    # nbatch 65 and 384: several chunks of slabs (gridDim.y > 1) added with float atomics -- still exact on integers
    g = R.gen(52)
    Lkp = (Lk + 31) // 32 * 32
    slabs = torch.full((nbatch, H, Lq, Lkp), float("nan"), dtype=torch.bfloat16)
    slabs[..., :Lk] = R.ints(g, -4, 4, nbatch, H, Lq, Lk, dtype=torch.bfloat16)
    dbias0 = R.ints(g, -9, 9, H, Lq, Lk)
    dbias = dbias0.cuda()
    ops.dbias_reduce(slabs.cuda(), dbias, nbatch=nbatch, H=H, Lq=Lq, Lk=Lk)
    torch.cuda.synchronize()
    want = dbias0.double() + slabs[..., :Lk].double().sum(0)
    assert torch.equal(dbias.cpu().double(), want)


# ------------------------------------------------------------------------------------------------- descriptor-table kernels
NTAB = [5, 1100]  # 1100 > 1024: the table is read from global memory instead of LDS


def _i64(rows):
    return torch.tensor(rows, dtype=torch.int64).cuda()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("n", NTAB)
def test_cast_pack_equals_torch_cast_with_ties_and_gaps(ops, n, dt):
    g = R.gen(61)
    lens = R.table_lengths(n, seed=61)
    src_off, src_total = R.layout(lens, lambda i: 4 * ((i * 5) % 3))
    dst_off, dst_total = R.layout(lens, lambda i: 4 * (i % 3))
    pre, total4 = R.prefix4(lens)
    src = R.with_bf16_ties(torch.randn(src_total, generator=g), g)
    srcd = src.cuda()
    desc = _i64([[srcd.data_ptr() + 4 * so, do, p4] for so, do, p4 in zip(src_off, dst_off, pre)])
    want = torch.full((dst_total,), -77.0, dtype=dt)
    dst = want.cuda()
    for so, do, ln in zip(src_off, dst_off, lens):
        want[do:do + ln] = src[so:so + ln].to(dt)
    ops.cast_pack(desc, total4, dst)
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), want)
    if dt == torch.bfloat16:  # the ties are there, in both parities, and went to the even neighbour
        tie = torch.zeros(src_total, dtype=torch.bool)
        tie[::5] = True
        lo, hi = src_off[1], src_off[1] + lens[1]
        t = src[lo:hi][tie[lo:hi]].view(torch.int32)
        assert len(t) >= 100 and bool(((t & 0xFFFF) == 0x8000).all()) and {0, 1} == set(((t >> 16) & 1).tolist())


@pytest.mark.parametrize("n", NTAB)
def test_quant_fp8_arena_equals_the_row_kernel(ops, n):
    g = R.gen(62)
    ks = [8, 64, 512, 4096]
    shapes = []  # (rows, K)
    for i in range(n):
        K = ks[3] if i % 211 == 3 else ks[2] if i % 37 == 2 else ks[int(torch.randint(0, 2, (1,), generator=g))]
        shapes.append((int(torch.randint(1, 9, (1,), generator=g)), K))
    lens = [r * K for r, K in shapes]
    offs, total = R.layout(lens, lambda i: 8 * (i % 3), align=8)
    arena = (torch.randn(total, generator=g) * 3).bfloat16()
    zero_t = min(2, n - 1)
    zr, zK = shapes[zero_t][0] - 1, shapes[zero_t][1]
    arena[offs[zero_t] + zr * zK:offs[zero_t] + (zr + 1) * zK] = 0  # one all-zero row: scale 1
    row0 = np.concatenate([[0], np.cumsum([r for r, _ in shapes])])
    desc = _i64([[off, r, K, int(r0)] for off, (r, K), r0 in zip(offs, shapes, row0[:-1])])
    want8 = torch.full((total,), 0xAB, dtype=torch.uint8)
    wants = torch.full((total // 8,), -5.0)
    ad = arena.cuda()
    for K in ks:  # the reference: klab_quant_fp8_rows (the same device function) on all rows of this width at once
        idx = [i for i in range(n) if shapes[i][1] == K]
        if not idx:
            continue
        rows = torch.cat([arena[offs[i]:offs[i] + lens[i]].view(-1, K) for i in idx])
        x8, sc = ops.quant_fp8_rows(rows.cuda())
        x8, sc, r = x8.cpu(), sc.cpu(), 0
        for i in idx:
            nr = shapes[i][0]
            want8[offs[i]:offs[i] + lens[i]] = x8[r:r + nr].reshape(-1)
            wants[offs[i] // 8:offs[i] // 8 + nr * (K // 8):K // 8] = sc[r:r + nr]
            r += nr
    assert float(wants[(offs[zero_t] + zr * zK) // 8]) == 1.0
    got8, gots = want8.clone().fill_(0xAB).cuda(), torch.full((total // 8,), -5.0).cuda()
    ops.quant_fp8_arena(desc, int(row0[-1]), ad, got8, gots)
    torch.cuda.synchronize()
    assert torch.equal(got8.cpu(), want8)
    assert torch.equal(gots.cpu(), wants)


# hyper-parameters that f32 holds exactly, 1 - beta included, so that the fp64 formula and the kernel start from the same numbers;
# step 3 of the bias corrections
ADAM = dict(lr=2.0 ** -9, beta1=0.875, beta2=1 - 2.0 ** -10, eps=1e-8)
ADAM["bias_corr1"] = 1 - ADAM["beta1"] ** 3
ADAM["bias_corr2"] = float(np.float32(1 - ADAM["beta2"] ** 3))


class AdamState:
    """n tensors as slices of flat buffers: p (with gaps), grads / m / v at goff (another layout with gaps), bf16 copies at aoff in
    an arena (every third tensor has none: aoff = -1).  The gaps and the arena start as sentinels / NaN."""

    def __init__(self, n, seed):
        g = R.gen(seed)
        self.lens = R.table_lengths(n, seed)
        self.poff, ptot = R.layout(self.lens, lambda i: 4 * (i % 2))
        self.goff, gtot = R.layout(self.lens, lambda i: 4 * ((i + 1) % 3))
        self.has_a = [i % 3 != 1 for i in range(n)]
        aoff, atot = R.layout([ln if h else 0 for ln, h in zip(self.lens, self.has_a)], lambda i: 4 * (i % 2))
        self.aoff = [a if h else -1 for a, h in zip(aoff, self.has_a)]
        self.pre, self.total4 = R.prefix4(self.lens)
        # magnitudes in [0.5, 2), m with the sign of g: m' = beta1 m + (1 - beta1) g' then has no cancellation and the relative bound on
        # m below follows from four roundings (|wd p| <= 0.02 cannot flip the sign of g')
        mag = lambda k: 0.5 + 1.5 * torch.rand(k, generator=g)
        sgn = lambda k: torch.randint(0, 2, (k,), generator=g).float() * 2 - 1
        self.p = mag(ptot) * sgn(ptot)
        self.g = mag(gtot) * sgn(gtot)
        self.m = mag(gtot) * self.g.sign()
        self.v = mag(gtot) ** 2
        self.arena = torch.full((max(atot, 4),), float("nan"), dtype=torch.bfloat16)

    def run(self, ops, wd, begin4=None, end4=None):
        pd, gd, md, vd, ad = self.p.cuda(), self.g.cuda(), self.m.cuda(), self.v.cuda(), self.arena.cuda()
        desc = _i64([[pd.data_ptr() + 4 * po, go, ao, p4] for po, go, ao, p4 in zip(self.poff, self.goff, self.aoff, self.pre)])
        ops.adam_step(desc, self.total4, gd, md, vd, ad, weight_decay=wd, begin4=begin4, end4=end4, **ADAM)
        torch.cuda.synchronize()
        assert torch.equal(gd.cpu(), self.g)
        return pd.cpu(), md.cpu(), vd.cpu(), ad.cpu()

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
        tensors = range(len(self.lens)) if tensors is None else tensors
        return torch.cat([flat[offs[i]:offs[i] + self.lens[i]] for i in tensors])


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.fixture(scope="module")
def adam_states():
    return {n: AdamState(n, seed=63) for n in NTAB}


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("n", NTAB)
def test_adam_step_matches_fp64_adam(ops, adam_states, n, wd):
    s = adam_states[n]
    p1, m1, v1, a1 = s.run(ops, wd)
    mp, mg, ma = s.masks(range(n))
    # nothing outside the tensors, nothing in the arena for tensors without a copy
    assert torch.equal(p1[~mp], s.p[~mp]) and torch.equal(m1[~mg], s.m[~mg]) and torch.equal(v1[~mg], s.v[~mg])
    assert torch.equal(_bits(a1)[~ma], _bits(s.arena)[~ma])
    P, P1 = s.gather(s.p, s.poff), s.gather(p1, s.poff)
    G, M, V = (s.gather(t, s.goff) for t in (s.g, s.m, s.v))
    M1, V1 = s.gather(m1, s.goff), s.gather(v1, s.goff)
    m_ref, v_ref, dp_ref = R.adam_ref(P, G, M, V, wd=wd, lr=ADAM["lr"], beta1=ADAM["beta1"], beta2=ADAM["beta2"], eps=ADAM["eps"],
                                      bc1=ADAM["bias_corr1"], bc2=ADAM["bias_corr2"])
    rm = float(((M1.double() - m_ref).abs() / m_ref.abs()).max())
    rv = float(((V1.double() - v_ref).abs() / v_ref.abs()).max())
    dp = P1.double() - P.double()
    rp = float(((dp - dp_ref).abs() / (1e-5 * dp_ref.abs() + 2 * U24 * P.double().abs())).max())
    print(f"adam n={n} wd={wd}: rel err m {rm / U24:.2f} ulp, v {rv / U24:.2f} ulp, dp err / bound {rp:.3e}")
    assert rm <= 4 * U24 and rv <= 4 * U24
    assert rp <= 1.0
    assert float(dp.abs().min()) > 0  # every element moved
    with_a = [i for i in range(n) if s.has_a[i]]
    assert torch.equal(s.gather(a1, s.aoff, with_a), s.gather(p1, s.poff, with_a).bfloat16())


@pytest.mark.parametrize("n", NTAB)
def test_adam_step_range_touches_only_its_tensors(ops, adam_states, n):
    s = adam_states[n]
    full = s.run(ops, 0.01)
    i0, i1 = (1, 4) if n == 5 else (n // 3, 2 * n // 3)
    part = s.run(ops, 0.01, begin4=s.pre[i0], end4=s.pre[i1])
    mp, mg, ma = s.masks(range(i0, i1))
    start = (s.p, s.m, s.v, s.arena)
    for got, whole, before, inside in zip(part, full, start, (mp, mg, mg, ma)):
        assert torch.equal(_bits(got)[inside], _bits(whole)[inside])    # the same update inside the range
        assert torch.equal(_bits(got)[~inside], _bits(before)[~inside])  # bit for bit untouched outside it
    assert not torch.equal(part[0][mp], s.p[mp])


# ------------------------------------------------------------------------------------------------------------------ ce_count
@pytest.mark.parametrize("rows", [1, 255, 257, 1000])
def test_ce_count_is_one_over_the_valid_labels(ops, rows):
    g = R.gen(71)
    labels = torch.randint(0, 32128, (rows,), generator=g)
    if rows > 1:
        labels[torch.rand(rows, generator=g) < 0.3] = -100
        labels[-1] = -100  # the tail a strided loop could miss
        labels[0] = 7
    n = int((labels != -100).sum())
    assert 0 < n <= rows
    inv = torch.full((1,), float("nan"), device="cuda")
    ops.ce_count(labels.cuda(), inv)
    assert float(inv.cpu()) == float(np.float32(1.0) / np.float32(n))
    # every label ignored: 0.0 (the documented departure from the reference's NaN)
    inv.fill_(float("nan"))
    ops.ce_count(torch.full((rows,), -100, dtype=torch.int64).cuda(), inv)
    assert float(inv.cpu()) == 0.0
