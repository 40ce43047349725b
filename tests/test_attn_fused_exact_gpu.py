"""klab_t5_attn_fused_fwd (RMS-norm -> q|k|v / q projection -> attention core, one launch) and klab_t5_attn_bwd_fused (o / co dgrad ->
delta -> single-pass attention backward, one launch) against exact references, per element.

Both kernels are otherwise only compared with the launches they replace under aggregate thresholds.  Here:
  * the dyadic fixtures of tests/exact_ref.py (every probability 0 or 1 / n; tests/test_exact_fixtures_cpu.py proves every stage
    exact and bf16-representable for exactly the tuples below): whatever is stored as bf16 -- xn, the projected q | k | v, ctx, dq,
    dk, dv, the stored-dS slab -- must be torch.equal to the fp64 reference; f32 outputs (lse, dbias through float atomics) within
    2^-20 of the magnitude of their terms; dbias through the slab is exact;
  * the backward kernel is handed dy and W, not dO: W is a signed permutation that sends rows of every k-tile of the dgrad into every
    head's column slice and dy = rows(dO) W^T, so a dropped or doubled k-tile, a wrong head slice or a swizzle mismatch between the
    W and dy reads changes the dO elements that depend on it;
  * the forward's x = sign * 2^k rows make xn = sign * gamma for every rstd inside the rstd bound, and every projection row has one
    +-1 per k-tile: the projected values are small integers in any summation order;
  * dropout at p = 0.5 (multiplier 0 or 2) against exact_ref.attn_drop_mult, the mask stated on its own;
  * shapes: 64 / 58 / 33 / 17 / 5 / 1 (self) and both sides of 32 (cross), B = 3 and B = 16 (the (B & 7) == 0 workgroup map), the
    forward also with six heads (inner = 384); every output in a sentinel buffer with a larger leading dimension and guard rows;
  * random operands once per kernel under per-element bounds counted from the roundings on each output's data path, each stage of the
    forward judged on the kernel's own previous output (DESIGN.md section 1 has the derivation and the measured worst ratios)."""
import pytest
import torch

from tests import exact_ref as R
from tests import rowops_ref as RR
from tests.attn_harness import (GUARD, PAD_VALUE, FlatOut, MatOut, assert_bf16_equal, assert_f32_close, first_bad, fused_input, ratio)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
D, DK = R.FUSED_D, R.FUSED_DK
MODES = ("atomics", "ds_ws", "ds_defer")


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


def shape_id(c):
    cross, B, H, Lq, Lk, causal = c
    return f"{'cross' if cross else 'self'}-B{B}-H{H}-{Lq}x{Lk}{'-causal' if causal else ''}"


def drop_id(d):
    return "nodrop" if d is None else f"drop{d[2]}"


def drop_kw(drop):
    if drop is None:
        return {}
    return dict(seed=torch.tensor([drop[0]], dtype=torch.int32).cuda(), tag=drop[1], drop_p=drop[2])


def assert_rows_equal(got, ref, what):
    """a [rows, columns] bf16 output against its fp64 reference, bit for bit in value"""
    want = R.to_bf16_via_f32(ref)
    bad = got != want
    if bool(bad.any()):
        i = first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong, first at (row, col) = {i}: got {float(got[i])}, want {float(want[i])}")
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------------------ backward
class BwdProblem:
    """device operands of klab_t5_attn_bwd_fused in the engine's layouts -- self: q | k | v in one [rows, 3 inner + 8] buffer and
    dq | dk | dv in another; cross: q and dq alone, k | v and dk | dv fused; ctx with a padded leading dimension; dy with `lddy`"""

    def __init__(self, cross, q, k, v, ctx, lse, dy, w, bias, causal, drop, lddy):
        self.cross, (self.B, self.H, self.Lq, _), self.Lk = cross, q.shape, k.shape[2]
        self.inner = self.H * DK
        if cross:
            _, ldq, (self.q,) = fused_input([q], BF16)
            _, ldkv, (self.k, self.v) = fused_input([k, v], BF16)
        else:
            _, ldq, (self.q, self.k, self.v) = fused_input([q, k, v], BF16)
            ldkv = ldq
        _, ldo, (self.ctx,) = fused_input([ctx], BF16)
        dyb = torch.full((dy.shape[0], lddy), PAD_VALUE, dtype=BF16)
        dyb[:, :D] = dy.to(BF16)
        self.dy = dyb.cuda()[:, :D]
        self.w = w.to(BF16).cuda()
        self.lse = lse.float().cuda()
        self.bias = None if bias is None else bias.float().cuda()
        self.kw = dict(B=self.B, H=self.H, Lq=self.Lq, Lk=self.Lk, dk=DK, bias=self.bias, causal=causal, ldq=ldq, ldk=ldkv, ldv=ldkv, ldo=ldo,
                       **drop_kw(drop))

    def outputs(self):
        if self.cross:
            dq, dkv = MatOut(self.B * self.Lq, self.inner, 1, BF16, self.H), MatOut(self.B * self.Lk, self.inner, 2, BF16, self.H)
            return (dq, dkv), (dq.views[0], dkv.views[0], dkv.views[1]), dict(lddq=dq.ld, lddk=dkv.ld, lddv=dkv.ld)
        o = MatOut(self.B * self.Lq, self.inner, 3, BF16, self.H)
        return (o,), tuple(o.views), dict(lddq=o.ld, lddk=o.ld, lddv=o.ld)

    def run(self, ops, mode):
        """mode: 'atomics' (dbias, no scratch), 'ds_ws' (stored dS + the reduce inside the call), 'ds_defer' (stored dS only;
        klab_dbias_reduce is called here, after the slab's pad columns have been poisoned: the reduce never reads them).
        -> dq, dk, dv [B, H, L, dk], dbias [H, Lq, Lk], ds [B, H, Lq, Lk] (the slab without its pad columns)"""
        B, H, Lq, Lk = self.B, self.H, self.Lq, self.Lk
        Lkp = (Lk + 31) // 32 * 32
        bufs, (dq, dk, dv), ld = self.outputs()
        dbias = FlatOut(H * Lq * Lk, torch.float32, fill=0.0)
        ds = FlatOut(B * H * Lq * Lkp, BF16) if mode != "atomics" else None
        ops.t5_attn_bwd_fused(self.dy, self.w, self.q, self.k, self.v, self.ctx, self.lse, dq, dk, dv, dbias=dbias.view,
                              ds_ws=None if ds is None else ds.view, ds_defer=mode == "ds_defer", **ld, **self.kw)
        if mode == "ds_defer":
            torch.cuda.synchronize()
            assert float(dbias.buf[GUARD:GUARD + dbias.n].abs().max()) == 0.0, "ds_defer must leave dbias to the caller"
            if Lkp > Lk:
                ds.view.view(B * H * Lq, Lkp)[:, Lk:] = float("nan")
            ops.dbias_reduce(ds.view, dbias.view, nbatch=B, H=H, Lq=Lq, Lk=Lk)
        torch.cuda.synchronize()
        out = {}
        if self.cross:
            out["dq"] = bufs[0].fetch(Lq)[0]
            out["dk"], out["dv"] = bufs[1].fetch(Lk)
        else:
            out["dq"], out["dk"], out["dv"] = bufs[0].fetch(Lq)
        out["dbias"] = dbias.fetch().reshape(H, Lq, Lk)
        if ds is not None:
            out["ds"] = ds.fetch().reshape(B, H, Lq, Lkp)[..., :Lk]
        return out


@pytest.mark.parametrize("drop", [None, R.FUSED_DROP], ids=drop_id)
@pytest.mark.parametrize("kind,n", R.fixtures_for(DK), ids=lambda v: str(v))
@pytest.mark.parametrize("shape", R.FUSED_SHAPES, ids=shape_id)
def test_backward_exact(ops, shape, kind, n, drop):
    cross, B, H, Lq, Lk, causal = shape
    f = R.fused_bwd_fixture(kind, n, cross, B, H, Lq, Lk, causal, drop)
    tag = f"{kind} n={n} {shape_id(shape)} {drop_id(drop)}"
    # the fixture's exact ctx / lse: the backward is judged on its own; lddy > 512 with the (B & 7) == 0 map
    pr = BwdProblem(cross, f.q, f.k, f.v, f.ctx, f.lse, R.dy_for(f.do), R.signed_perm()[0], f.bias, causal, drop, lddy=D + 8 if B == 16 else D)
    absds = f.dS.abs()
    for mode in MODES:
        got = pr.run(ops, mode)
        for name, ref in (("dq", f.dq), ("dk", f.dk_), ("dv", f.dv)):
            assert_bf16_equal(got[name], ref, f"backward {name} ({mode}), {tag}")
        if "ds" in got:
            assert_bf16_equal(got["ds"], f.dS, f"stored dS ({mode}), {tag}")
            bad = got["dbias"].double() != f.dbias  # a sum of exact bf16 values in f32: exact
            assert not bool(bad.any()), f"backward dbias ({mode}), {tag}: first wrong (h, q, key) = {first_bad(bad) if bool(bad.any()) else None}"
        else:
            assert_f32_close(got["dbias"], f.dbias, f"backward dbias ({mode}), {tag}", absds.sum(0))


def test_backward_envelope_declines_without_writing(ops):
    cross, B, H, Lq, Lk, causal = False, 3, 8, 17, 17, False
    f = R.fused_bwd_fixture("q0", 2, cross, B, H, Lq, Lk, causal, None)
    pr = BwdProblem(cross, f.q, f.k, f.v, f.ctx, f.lse, R.dy_for(f.do), R.signed_perm()[0], f.bias, causal, None, lddy=D)
    (o,), (dq, dk, dv), ld = pr.outputs()
    dbias, ds = FlatOut(H * Lq * Lk, torch.float32, fill=0.0), FlatOut(B * H * Lq * 32, BF16)
    extra = dict(dbias=dbias.view, ds_ws=ds.view, **ld)
    args = (pr.q, pr.k, pr.v, pr.ctx, pr.lse)
    calls = {
        "Lk = 65": lambda: ops.t5_attn_bwd_fused(pr.dy, pr.w, *args, dq, dk, dv, **extra, **dict(pr.kw, Lk=65, bias=None)),
        "d_model = 256": lambda: ops.t5_attn_bwd_fused(pr.dy[:, :256].contiguous(), pr.w[:256].contiguous(), *args, dq, dk, dv, **extra, **pr.kw),
        "H * dk != 512": lambda: ops.t5_attn_bwd_fused(pr.dy, pr.w, *args, dq, dk, dv, **extra, **dict(pr.kw, H=6)),
        "misaligned dq": lambda: ops.t5_attn_bwd_fused(pr.dy, pr.w, *args, o.buf[1:, 1:], dk, dv, **extra, **pr.kw),
    }
    for what, call in calls.items():
        with pytest.raises(NotImplementedError):
            call()
        torch.cuda.synchronize()
        for buf in (o, dbias, ds):
            buf.assert_untouched(f"klab_t5_attn_bwd_fused declined ({what})")


# ------------------------------------------------------------------------------------------------------------------- forward
def run_forward(ops, cross, B, H, Lq, Lk, causal, drop, x, gamma, w, k, v, bias):
    """-> xn [B Lq, 512] bf16, rstd [B Lq], the projected blocks ([B Lq, inner] each: q | k | v, or q), ctx [B, H, Lq, 64], lse [B, H, Lq];
    every output from a sentinel buffer (proj and ctx with padded leading dimensions and guard rows, xn / rstd / lse between guards)"""
    inner = H * DK
    xd, gd, wd = x.float().cuda(), gamma.float().cuda(), w.to(BF16).cuda()
    xn, rstd = FlatOut(B * Lq * D, BF16), FlatOut(B * Lq, torch.float32)
    proj = MatOut(B * Lq, inner, 1 if cross else 3, BF16, H)
    ctx, lse = MatOut(B * Lq, inner, 1, BF16, H), FlatOut(B * H * Lq, torch.float32)
    kv = {}
    if cross:
        _, ldkv, (kd, vd) = fused_input([k, v], BF16)
        kv = dict(k=kd, v=vd, ldk=ldkv, ldv=ldkv)
    ops.t5_attn_fused_fwd(xd, gd, wd, xn.view.view(B * Lq, D), rstd.view, proj.views[0], ctx.views[0], lse.view, B=B, H=H, Lq=Lq, Lk=Lk, dk=DK,
                          bias=None if bias is None else bias.float().cuda(), causal=causal, cross=cross, **kv, **drop_kw(drop))
    torch.cuda.synchronize()
    return xn.fetch().reshape(B * Lq, D), rstd.fetch(), proj.fetch_rows(), ctx.fetch(Lq)[0], lse.fetch().reshape(B, H, Lq)


@pytest.mark.parametrize("drop", [None, R.FUSED_DROP], ids=drop_id)
@pytest.mark.parametrize("kind,n", R.FUSED_FWD_KINDS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", R.FUSED_FWD_SHAPES, ids=shape_id)
def test_forward_exact(ops, shape, kind, n, drop):
    cross, B, H, Lq, Lk, causal = shape
    f = R.fused_fwd_fixture(kind, n, cross, B, H, Lq, Lk, causal, drop)
    tag = f"{kind} n={n} {shape_id(shape)} {drop_id(drop)}"
    xn, rstd, proj, ctx, lse = run_forward(ops, cross, B, H, Lq, Lk, causal, drop, f.x, f.gamma, f.w, f.k, f.v, f.bias)
    # complete for every sample: only the head-0 workgroup of a sample writes them
    assert_rows_equal(xn, f.xn, f"xn, {tag}")
    RR.assert_within("rstd", rstd, f.rstd, R.rstd_bound(f.rstd), ", " + tag)
    inner = H * DK
    for blk, name in enumerate(("q",) if cross else ("q", "k", "v")):
        assert_rows_equal(proj[blk], f.proj[:, blk * inner:(blk + 1) * inner], f"projected {name} (head h at column {blk} * inner + 64 h), {tag}")
    assert_bf16_equal(ctx, f.ctx, f"ctx, {tag}")
    assert_f32_close(lse, f.lse, f"lse, {tag}")


# ------------------------------------------------------------------------------------------- random operands, per element
def causal_zero(x, Lq, Lk):
    return x.masked_fill((torch.arange(Lk)[None, :] > torch.arange(Lq)[:, None])[None, None], 0.0)


@pytest.mark.parametrize("drop", [None, R.FUSED_RANDOM_DROP], ids=drop_id)
@pytest.mark.parametrize("shape", R.FUSED_RANDOM, ids=shape_id)
def test_forward_random_operands_per_element(ops, shape, drop):
    cross, B, H, Lq, Lk, causal = shape
    d = R.fused_randn(cross, B, H, Lq, Lk)
    print(f"\nfused forward randn {shape_id(shape)} {drop_id(drop)}")
    xn, rstd, proj, ctx, lse = run_forward(ops, cross, B, H, Lq, Lk, causal, drop, d["x"], d["gamma"], d["w"], d["k"], d["v"], d["bias"])
    # each stage on the kernel's own previous output
    r64 = (d["x"].pow(2).mean(-1) + 1e-6).rsqrt()
    worst = [ratio(rstd, r64, R.rstd_bound(r64), "rstd")]
    want = RR.rms_fwd_from_stat(d["x"].float(), d["gamma"].float(), rstd).to(BF16)  # g * (x * rs): two f32 multiplies, nothing to contract
    bad = xn != want
    assert not bool(bad.any()), f"xn from the kernel's own rstd: {int(bad.sum())} elements wrong, first at (row, col) = {first_bad(bad) if bool(bad.any()) else None}"
    xn64 = xn.double()
    got_proj = torch.cat(proj, 1)
    pref = xn64 @ d["w"].T
    worst.append(ratio(got_proj, pref, R.gemm_bound(xn64.abs() @ d["w"].abs().T, D, pref, bf16_out=True), "proj"))
    q = R.heads(proj[0].double(), Lq, H)
    k, v = (d["k"], d["v"]) if cross else (R.heads(proj[1].double(), Lk, H), R.heads(proj[2].double(), Lk, H))
    _, lref, P = R.attn_reference(q, k, v, d["bias"], causal)
    Pm = P if drop is None else P * R.attn_drop_mask(*drop, B, H, Lq, Lk)
    cref = Pm @ v
    f32b = R.attn_f32_bounds(dict(P=Pm, D=Pm), q, k, v, torch.zeros_like(q), Lq, Lk, DK, B)["ctx"]
    worst.append(ratio(ctx, cref, R.attn_fwd_bound(Pm, v) + f32b, "ctx"))
    f32f = R.attn_f32_factor(q, k, Lk, DK)
    vis = causal_zero(f32f, Lq, Lk) if causal else f32f
    worst.append(ratio(lse, lref, vis.amax(-1) + 4.0 * R.U24 * lref.abs(), "lse"))
    bad = [msg for v_, msg in worst if not v_ <= 1.0]
    assert not bad, bad


@pytest.mark.parametrize("drop", [None, R.FUSED_RANDOM_DROP], ids=drop_id)
@pytest.mark.parametrize("shape", R.FUSED_RANDOM, ids=shape_id)
def test_backward_random_operands_per_element(ops, shape, drop):
    cross, B, H, Lq, Lk, causal = shape
    d = R.fused_randn(cross, B, H, Lq, Lk)
    inner = H * DK
    q, k, v, bias = d["q"], d["k"], d["v"], d["bias"]
    print(f"\nfused backward randn {shape_id(shape)} {drop_id(drop)}")
    # what the forward leaves behind: klab_t5_attn_fwd's ctx (bf16) and lse (f32), under the same mask
    qd, kd, vd = (R.unheads(t).to(BF16).cuda() for t in (q, k, v))
    ctx_d, lse_d = torch.zeros(B * Lq, inner, dtype=BF16, device="cuda"), torch.zeros(B, H, Lq, device="cuda")
    ops.t5_attn_fwd(qd, kd, vd, ctx_d, lse_d, B=B, H=H, Lq=Lq, Lk=Lk, dk=DK, bias=bias.float().cuda(), causal=causal, **drop_kw(drop))
    torch.cuda.synchronize()
    ctx64, lse64 = R.heads(ctx_d.cpu().double(), Lq, H), lse_d.cpu().double()
    M = torch.ones(B, H, Lq, Lk, dtype=torch.float64) if drop is None else R.attn_drop_mask(*drop, B, H, Lq, Lk)
    do = R.heads(d["dy"] @ d["wo"], Lq, H)                  # dense K = 512 accumulation of the dgrad phase is judged here
    absdo = R.heads(d["dy"].abs() @ d["wo"].abs(), Lq, H)
    r = R.attn_backward_reference(q, k, v, bias, causal, ctx64, lse64, do, M)
    pr = BwdProblem(cross, q, k, v, ctx64, lse64, d["dy"], d["wo"], bias, causal, drop, lddy=D + 8 if B == 16 else D)
    worst = []
    for mode in ("ds_ws", "atomics"):
        got = pr.run(ops, mode)
        bnd = R.attn_bwd_fused_bounds(r, M, q, k, v, ctx64, do, absdo, Lq, Lk, DK, B, stored_ds="ds" in got)
        for name in ("dq", "dk", "dv", "dbias"):
            worst.append(ratio(got[name], r[name], bnd[name], f"{name} ({mode})"))
    bad = [msg for v_, msg in worst if not v_ <= 1.0]
    assert not bad, bad
