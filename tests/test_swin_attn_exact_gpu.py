"""Swin-V2 window attention against tests/swin_exact_ref.py: exact fixtures (torch.equal on bf16 outputs, 2^-20 on f32 outputs),
random operands under a per-element bound, and the memory contract of every output (guard bands, overwrite / accumulate).

Dispatcher rule -> shape (B = 2 throughout; the lists are swin_exact_ref.SMALL_GEO / SMALL_CFG / LARGE_GEO / FUSED_GEO):

  klab_swin_attn_fwd, n <= 64, R % w == 0, dense bias
    f32, hd 16 / 32   swin_attn_fwd_kernel<float, 16 / 32>        C = 32 / 64, H = 2
    bf16, hd 16       swin_attn_fwd_kernel<bf16, 16>              C = 32
    bf16, hd 32       swin_attn_fwd_mfma32                        C = 64   (swin_attn_fwd_kernel<bf16, 32> is unreachable)
    window sizes      w = 2 (R = 2: one window, H = 8; R = 4 shifted), w = 4 (R = 8: all four window classes; R = 12: an interior
                      window), w = 7 (49 keys padded to 64), w = 8 (exactly one tile), each with shift 0 and shift > 0
  klab_swin_attn_bwd, same shapes
    mfma=False        swin_attn_bwd_kernel<T, HD>, all four (dtype, hd)
    mfma=True         bf16, hd 32 (swin_bwd_mfma_ok): gather -> t5_attn_bwd_mfma<32> -> klab_dbias_reduce -> scatter, with
                      swin_bias_mask_kernel when shift > 0, with and without dbias
  swin_use_large: n > 64 (w = 9: 64 + 17 keys; w = 12: 144), R % w != 0 (R = 9 / w = 4, R = 10 / w = 6), or a bias table
    mfma=False        swin_attn_fwd_tiled / _bwd_dq_tiled / _bwd_dkv_tiled<T, HD>, all four (dtype, hd), dense and table bias
    mfma=True         bf16, hd 32, table (swin_flash_ok): the streaming matrix-core kernels, forward and both backward passes
  klab_swin_qkv_attn_fused / _img: C = 64, 128 (weights in registers), 256 (k block by k block); w = 7, 8; shift 0 / > 0; bqkv or not
"""
import math

import pytest
import torch

from tests import swin_exact_ref as S

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
SENT = 96.0      # guard-band content (a bf16 number)
PAD = 256        # guard elements on each side
B = S.B_
U20 = 2.0 ** -20

# Margins of the per-element bounds over the first-order expressions of SwinBounds, per (operand dtype, output).  The worst measured
# |kernel - fp64| / expression over all cases of this file is recorded per kernel in DESIGN.md section 1 and repeated here; each
# margin is at most 4x the worst ratio of its row.  f32: the expressions add every rounding linearly, the kernels' errors add like
# a random walk, hence margins far below 1.  bf16: the output rounding and an operand rounding flip of q-hat / k-hat are met
# exactly by some element (ratio 0.97 .. 0.99).  f32 dv_bias stays below the allowance for the initial content (no ratio to
# measure): it takes d(bias table)'s margin.
MARGIN = {
    "f32": dict(ctx=0.1, lse=0.25, dqkv=0.2, dls=0.01, dbias=0.078, dtable=0.018, dv_bias=0.018),
    #   measured: ctx 0.029, lse 0.070, dqkv 0.057, dls 0.003, dbias 0.020, dtable 0.005, dv_bias -
    "bf16": dict(ctx=2.0, lse=2.0, dqkv=2.0, dls=0.125, dbias=2.0, dtable=1.0, dv_bias=0.75),
    #   measured: ctx 0.983, lse 0.993, dqkv 0.974, dls 0.045, dbias 0.525, dtable 0.362, dv_bias 0.197 (fused kernels: ctx 0.617)
}


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


class Guarded:
    """a tensor inside a larger buffer filled with a sentinel before and after"""

    def __init__(self, shape, dtype, init=None):
        numel = int(math.prod(shape))
        self.buf = torch.full((numel + 2 * PAD,), SENT, dtype=dtype, device="cuda")
        self.t = self.buf[PAD:PAD + numel].view(*shape)
        self.t.fill_(float("nan") if init is None else init)   # NaN: an element the kernel does not write shows up
        self.numel = numel

    def intact(self):
        return bool((self.buf[:PAD] == SENT).all()) and bool((self.buf[PAD + self.numel:] == SENT).all())

    def cpu(self):
        return self.t.detach().cpu().double()


def first_bad(bad):
    idx = bad.nonzero()[0].tolist()
    return idx, int(bad.sum())


def assert_exact(name, got, want, f32=False, where=None):
    """bf16 outputs: equal bit for bit (as numbers); f32 outputs: within 2^-20 of the tensor's largest magnitude"""
    bad = (got - want).abs() > U20 * float(want.abs().max()) if f32 else ~(got == want)
    if where is not None:
        bad = bad & where
    if bool(bad.any()):
        idx, cnt = first_bad(bad)
        raise AssertionError(f"{name}: {cnt} wrong elements, first at {idx}: got {got[tuple(idx)].item()!r}, want {want[tuple(idx)].item()!r}")


def assert_bound(dn, name, got, want, bound, extra=0.0):
    """|got - want| <= margin * bound + extra, element by element (extra: the rounding an accumulated output suffers at the
    magnitude of its initial content, which is no property of the kernel)"""
    m = MARGIN[dn][name]
    ratio = (((got - want).abs() - extra).clamp_min(0.0) / bound.clamp_min(1e-300))
    ratio = torch.where((got - want).abs() == 0, torch.zeros_like(ratio), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"RATIO {name} {worst:.4f}")     # against the expression, before the margin
    bad = ~(ratio <= m)
    if bool(bad.any()):
        idx, cnt = first_bad(bad)
        raise AssertionError(f"{name}: {cnt} elements outside the bound (worst ratio {worst:.3f}, margin {m}), first at {idx}: got "
                             f"{got[tuple(idx)].item()!r}, want {want[tuple(idx)].item()!r}, bound {m * bound[tuple(idx)].item()!r}")


INIT = dict(dbias=3.0, dtable=-5.0, dls=-2.0, dv_bias=7.0)   # accumulated outputs start from a nonzero integer


def run(ops, dt, geo, d, mfma, backward=True, want_dbias=True):
    """forward (+ backward) of the public entry points on guarded outputs; d: fp64 qkv, dctx, ls, bias | table, v_bias"""
    Bq, R, w, shift, H, C = geo
    n = w * w
    nW = S.geom(R, w)[2]
    cu = lambda x, t=None: None if x is None else x.to(t or torch.float32).cuda()
    qkv, dctx = cu(d["qkv"], dt), cu(d["dctx"], dt)
    bias, table, ls, vb = cu(d["bias"]), cu(d["table"]), cu(d["ls"]), cu(d["v_bias"])
    kw = dict(B=Bq, R=R, w=w, shift=shift, H=H, C=C)
    out = dict(ctx=Guarded((Bq * R * R, C), dt), lse=Guarded((Bq * nW, H, n), torch.float32))
    ops.swin_attn_fwd(qkv, out["ctx"].t, bias, ls, out["lse"].t, bias_table=table, mfma=mfma, v_bias=vb, **kw)
    if backward:
        out["dqkv"] = Guarded((Bq * R * R, 3 * C), dt)
        out["dls"] = Guarded((H,), torch.float32, INIT["dls"])
        if table is not None:
            out["dtable"] = Guarded(((2 * w - 1) ** 2, H), torch.float32, INIT["dtable"])
        elif want_dbias:
            out["dbias"] = Guarded((H, n, n), torch.float32, INIT["dbias"])
        if vb is not None:
            out["dv_bias"] = Guarded((C,), torch.float32, INIT["dv_bias"])
        g = lambda k: out[k].t if k in out else None
        ops.swin_attn_bwd(qkv, out["ctx"].t, bias, ls, out["lse"].t, dctx, out["dqkv"].t, g("dbias"), out["dls"].t, bias_table=table,
                          dbias_table=g("dtable"), v_bias=vb, dv_bias=g("dv_bias"), mfma=mfma, **kw)
    torch.cuda.synchronize()
    for k, v in out.items():
        assert v.intact(), f"{k}: the kernel wrote outside its output"
    return {k: v.cpu() for k, v in out.items()}


def fixture_inputs(f):
    return dict(qkv=f.qkv, dctx=f.dctx, ls=f.ls, bias=f.bias, table=f.table, v_bias=f.v_bias)


def check_lse_exact(f, lse):
    """single-key rows on heads whose scale is exactly 1: lse == score (needs __logf(1) == 0 and __expf(0) == 1, which this
    asserts of the kernels); every other real row within 2^-20"""
    real = f.real[:, None, :].expand_as(f.lse)
    assert not bool(torch.isnan(lse[real]).any()), "lse: a real row was not written"
    unit = (f.ls == 0).view(1, -1, 1).expand_as(f.lse)
    assert_exact("lse (single-key rows)", lse, f.lse, where=real & f.single & unit)
    # (a clamped head's scale is __expf(ln 100): a few ulp of 100, hence 8 x 2^-20 there)
    bad = ((lse - f.lse).abs() > U20 * torch.where(unit, 1.0, 8.0) * f.lse.abs().clamp_min(1.0)) & real
    if bool(bad.any()):
        idx, cnt = first_bad(bad)
        raise AssertionError(f"lse: {cnt} wrong rows, first at (window, head, row) {idx}: got {lse[tuple(idx)].item()!r}, want {f.lse[tuple(idx)].item()!r}")


def check_select(f, o, dt):
    f32 = dt == torch.float32
    assert_exact("ctx", o["ctx"], f.ctx, f32)
    check_lse_exact(f, o["lse"])
    assert_exact("dqkv", o["dqkv"], f.dqkv, f32)
    # accumulated outputs: initial content + gradient; d logit_scale is exactly 0 here (sum_j dS_ij = 0 over keys of equal cosine)
    assert_exact("dlogit_scale", o["dls"], torch.full_like(f.dls, INIT["dls"]))
    if "dbias" in o:
        assert_exact("dbias", o["dbias"], f.dbias + INIT["dbias"], True)
    if "dtable" in o:
        assert_exact("dbias_table", o["dtable"], f.dtable + INIT["dtable"], True)
    if "dv_bias" in o:
        assert_exact("dv_bias", o["dv_bias"], f.dv_bias + INIT["dv_bias"], True)


# ---- 2. exact fixtures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn,R,w,shift,H,C", S.small_cases(), ids=lambda v: str(v))
def test_small_window_select_fixture_is_exact(ops, dn, R, w, shift, H, C):
    dt = DT[dn]
    f = S.swin_fixture("select", B, R, w, shift, H, C, "dense")
    geo = (B, R, w, shift, H, C)
    check_select(f, run(ops, dt, geo, fixture_inputs(f), mfma=False), dt)
    if dn == "bf16" and C == H * 32:   # the matrix-core backward, with and without the bias gradient
        check_select(f, run(ops, dt, geo, fixture_inputs(f), mfma=True), dt)
        o = run(ops, dt, geo, fixture_inputs(f), mfma=True, want_dbias=False)
        assert "dbias" not in o
        check_select(f, o, dt)


@pytest.mark.parametrize("dn,R,w,shift,H,C,form,mfma", S.large_cases(), ids=lambda v: str(v))
def test_large_and_padded_window_select_fixture_is_exact(ops, dn, R, w, shift, H, C, form, mfma):
    dt = DT[dn]
    f = S.swin_fixture("select", B, R, w, shift, H, C, form)
    check_select(f, run(ops, dt, (B, R, w, shift, H, C), fixture_inputs(f), mfma=mfma), dt)


@pytest.mark.parametrize("dn,R,w,shift,H,C", S.region_cases(), ids=lambda v: str(v))
def test_zero_bias_probabilities_are_one_over_the_region_size(ops, dn, R, w, shift, H, C):
    dt = DT[dn]
    f = S.swin_fixture("region", B, R, w, shift, H, C)
    o = run(ops, dt, (B, R, w, shift, H, C), fixture_inputs(f), mfma=True, backward=False)
    assert_exact("ctx", o["ctx"], f.ctx, dt == torch.float32)
    check_lse_exact(f, o["lse"])


@pytest.mark.parametrize("dn,R,w,shift,H,C,mfma", S.REGION_TABLE + [c + (False,) for c in S.region_cases()], ids=lambda v: str(v))
def test_zero_bias_every_pair_of_a_region_reaches_the_bias_gradient(ops, dn, R, w, shift, H, C, mfma):
    """the select fixtures leave most (query, key) pairs without a gradient; here every pair of a region has one, and the f32 bias
    gradients (table form: tiled and streaming kernels; dense form: the vector-ALU backward) are short dyadic sums"""
    dt = DT[dn]
    form = "table" if (dn, R, w, shift, H, C, mfma) in S.REGION_TABLE else "dense"
    f = S.swin_fixture("region", B, R, w, shift, H, C, form)
    o = run(ops, dt, (B, R, w, shift, H, C), fixture_inputs(f), mfma=mfma)
    assert_exact("ctx", o["ctx"], f.ctx, dt == torch.float32)
    if form == "table":
        assert_exact("dbias_table", o["dtable"], f.dtable + INIT["dtable"], True)
    else:
        assert_exact("dbias", o["dbias"], f.dbias + INIT["dbias"], True)
    assert_exact("dlogit_scale", o["dls"], torch.full_like(f.dls, INIT["dls"]))


@pytest.mark.parametrize("dn,R,w,shift,H,C,perm", S.onehot_cases(), ids=lambda v: str(v))
def test_selection_by_the_scores_alone_is_exact(ops, dn, R, w, shift, H, C, perm):
    dt = DT[dn]
    f = S.swin_fixture("onehot", B, R, w, shift, H, C, perm=perm)
    o = run(ops, dt, (B, R, w, shift, H, C), fixture_inputs(f), mfma=True, backward=False)
    assert_exact("ctx", o["ctx"], f.ctx, dt == torch.float32)
    check_lse_exact(f, o["lse"])


def fused_run(ops, x, wq, bq, bias, ls, geo):
    """both projection kernels on guarded outputs (and the bias image in a guarded buffer): (ctx, ctx_img, image)"""
    from klab_multimodalmodel_amd import _lib as L
    Bq, R, w, shift, H, C = geo
    bf = torch.bfloat16
    xg, wg = x.to(bf).cuda(), wq.to(bf).cuda()
    bg = None if bq is None else bq.float().cuda()
    biasg, lsg = bias.float().cuda(), ls.float().cuda()
    kw = dict(B=Bq, R=R, w=w, shift=shift, H=H, C=C)
    c1, c2 = Guarded((Bq * R * R, C), bf), Guarded((Bq * R * R, C), bf)
    ops.swin_qkv_attn_fused(xg, wg, bg, c1.t, biasg, lsg, **kw)
    lib = L.load()
    nbytes = lib.klab_swin_bias_image_bytes(w, shift, H)
    img = Guarded((nbytes // 4,), torch.float32)
    L.check(lib.klab_swin_bias_image(biasg.data_ptr(), img.t.data_ptr(), R, w, shift, H, L.stream_ptr()), "klab_swin_bias_image")
    ops.swin_qkv_attn_fused_img(xg, wg, bg, c2.t, img.t.view(-1, H, 4, 64, 16), lsg, **kw)
    torch.cuda.synchronize()
    assert c1.intact() and c2.intact() and img.intact(), "a fused kernel or the image builder wrote outside its output"
    assert not bool(torch.isnan(img.t).any())
    return c1.cpu(), c2.cpu(), img.cpu()


FUSED = [(R, w, s, C, wb) for (R, w, s) in S.FUSED_GEO for C in S.FUSED_C for wb in (False, True)]


@pytest.mark.parametrize("R,w,shift,C,with_b", FUSED, ids=lambda v: str(v))
def test_fused_projection_kernels_are_exact(ops, R, w, shift, C, with_b):
    H = C // 32
    kinds = ("select", "onehot") + (("region",) if shift > 0 and w == 8 else ())
    for kind in kinds:
        f = S.swin_fixture(kind, B, R, w, shift, H, C, "dense", True)
        x, wq = f.fused_operands()
        bq, want = None, f.ctx
        if with_b and kind != "region":   # k part zero as in the model; a q bias would break the one-hot codes, the v bias is +-1
            bq = torch.cat([torch.zeros(2 * C, dtype=torch.float64), torch.tensor([1.0, -1.0] * (C // 2), dtype=torch.float64)])
            want = f.ctx + bq[2 * C:]
        bias = f.bias if f.bias is not None else torch.zeros(H, w * w, w * w, dtype=torch.float64)
        c1, c2, _img = fused_run(ops, x, wq, bq, bias, f.ls, (B, R, w, shift, H, C))
        assert_exact(f"{kind}: ctx (dense bias)", c1, want)
        assert_exact(f"{kind}: ctx (bias image)", c2, want)


def test_bias_image_holds_bias_mask_and_padding(ops):
    """every float of the image of klab_swin_bias_image against the layout klab_mm.h documents, built here from the reference's
    regions: [class, head, query tile, lane, 16] with query = 16 qt + lane % 16, key = 16 t + 4 (lane / 16) + r"""
    for R, w, shift, H in [(14, 7, 3, 2), (16, 8, 4, 3), (14, 7, 0, 2), (8, 4, 2, 2)]:
        n = w * w
        bias = (16 * torch.sigmoid(torch.randn(H, n, n, generator=S.gen(w)))).float()
        from klab_multimodalmodel_amd import _lib as L
        lib = L.load()
        img = Guarded((lib.klab_swin_bias_image_bytes(w, shift, H) // 4,), torch.float32)
        bg = bias.cuda()
        L.check(lib.klab_swin_bias_image(bg.data_ptr(), img.t.data_ptr(), R, w, shift, H, L.stream_ptr()), "klab_swin_bias_image")
        torch.cuda.synchronize()
        assert img.intact()
        ncls = 4 if shift > 0 else 1
        got = img.cpu().view(ncls, H, 4, 64, 4, 4)
        reg = S.region_ids(R, w, shift)
        nWr = R // w
        lane = torch.arange(64)
        q = (torch.arange(4)[:, None] * 16 + (lane % 16)[None, :])[:, :, None, None]          # [qt, lane, 1, 1]
        key = (torch.arange(4)[:, None] * 16 + torch.arange(4)[None, :])[None, None] + (lane // 16 * 4)[None, :, None, None]
        q, key = q.expand(4, 64, 4, 4), key.expand(4, 64, 4, 4)
        qc, kc = q.clamp_max(n - 1), key.clamp_max(n - 1)
        for cls in range(ncls):
            win = ((nWr - 1) * nWr if cls & 2 else 0) + (nWr - 1 if cls & 1 else 0)
            other = reg[win][qc] != reg[win][kc]
            want = bias.double()[:, qc, kc] + other.double()[None] * -200.0
            want = torch.where((key < n)[None].expand_as(want), want, torch.full_like(want, -math.inf))
            assert_exact(f"image class {cls}", got[cls], want.float().double())


# ---- 3. random operands: every element under its own bound ---------------------------------------------------------------------
def check_random(ops, dn, geo, form, mfma_fwd, mfma):
    dt = DT[dn]
    Bq, R, w, shift, H, C = geo
    d = S.swin_randn(Bq, R, w, shift, H, C, form)
    r = S.swin_randn_reference(Bq, R, w, shift, H, C, form, dn)
    o = run(ops, dt, geo, d, mfma=mfma)
    fb = S.SwinBounds(r, *geo, dt, mfma=mfma_fwd)
    bb = S.SwinBounds(r, *geo, dt, mfma=mfma) if mfma != mfma_fwd else fb
    real = r["real"][:, None, :].expand_as(r["lse"])
    assert_bound(dn, "ctx", o["ctx"], r["ctx"], fb.ctx())
    assert not bool(torch.isnan(o["lse"][real]).any())
    assert_bound(dn, "lse", torch.where(real, o["lse"], r["lse"]), r["lse"], fb.e_lse)
    assert_bound(dn, "dqkv", o["dqkv"], r["dqkv"], bb.dqkv())
    assert_bound(dn, "dls", o["dls"] - INIT["dls"], r["dls"], bb.dls, U24_INIT * abs(INIT["dls"]))
    if H >= 2:
        assert float(o["dls"][0]) == INIT["dls"]        # logit_scale 5.0 is clamped: no gradient, whatever dS is
    if "dbias" in o:
        assert_bound(dn, "dbias", o["dbias"] - INIT["dbias"], r["dbias"], bb.dbias, U24_INIT * abs(INIT["dbias"]))
    if "dtable" in o:
        assert_bound(dn, "dtable", o["dtable"] - INIT["dtable"], r["dtable"], bb.dtable(), U24_INIT * abs(INIT["dtable"]))
    if "dv_bias" in o:
        assert_bound(dn, "dv_bias", o["dv_bias"] - INIT["dv_bias"], r["dv_bias"], bb.dv_bias(), U24_INIT * abs(INIT["dv_bias"]))


U24_INIT = 2.0 ** -20   # an accumulated f32 output that starts from INIT rounds at INIT's magnitude on every addition it receives (up to 18 windows)


@pytest.mark.parametrize("dn,R,w,shift,H,C", S.small_cases(), ids=lambda v: str(v))
def test_small_window_random_operands_within_the_per_element_bound(ops, dn, R, w, shift, H, C):
    geo = (B, R, w, shift, H, C)
    mm = dn == "bf16" and C == H * 32        # the forward is the matrix-core kernel whatever the backward is
    check_random(ops, dn, geo, "dense", mm, False)
    if mm:
        check_random(ops, dn, geo, "dense", True, True)


@pytest.mark.parametrize("dn,R,w,shift,H,C,form,mfma", S.large_cases(), ids=lambda v: str(v))
def test_large_and_padded_window_random_operands_within_the_per_element_bound(ops, dn, R, w, shift, H, C, form, mfma):
    check_random(ops, dn, (B, R, w, shift, H, C), form, mfma, mfma)


@pytest.mark.parametrize("R,w,shift,C,with_b", FUSED, ids=lambda v: str(v))
def test_fused_projection_random_operands_within_the_per_element_bound(ops, R, w, shift, C, with_b):
    H = C // 32
    n = w * w
    g = S.gen(9000 + C + w + shift)
    rb = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).double()
    x, wq = rb(B * R * R, C), (rb(3 * C, C) / math.sqrt(C)).to(torch.bfloat16).double()
    bq = None
    if with_b:
        bq = (0.5 * torch.randn(3 * C, generator=g)).float().double()
        bq[C:2 * C] = 0
    bias = (16 * torch.sigmoid(torch.randn(H, n, n, generator=g))).float().double()
    ls = (math.log(10.0) + 0.3 * torch.randn(H, generator=g)).float().double()
    ls[0] = 5.0
    qkv = S.fused_qkv(x, wq, bq)
    r = S.swin_reference(qkv, ls, B, R, w, shift, H, C, bias, round_dtype=torch.bfloat16)
    # f32 error of the projection (C exact products summed in the matrix unit), per row relative to |q|, |k|
    err = 2.0 * S.U24 * (C + 2) * (x.abs() @ wq.abs().T + (0.0 if bq is None else bq.abs()[None]))
    ew = S.to_windows(err, B, R, w, shift)
    eq = S.heads(ew[..., :C], H).amax(-1) / r["qn"].clamp_min(1e-300)
    ek = S.heads(ew[..., C:2 * C], H).amax(-1) / r["kn"].clamp_min(1e-300)
    bound = S.SwinBounds(r, B, R, w, shift, H, C, torch.bfloat16, mfma=True, eq=eq, ek=ek, v_rounded=True).ctx()
    c1, c2, _img = fused_run(ops, x, wq, bq, bias, ls, (B, R, w, shift, H, C))
    assert_bound("bf16", "ctx", c1, r["ctx"], bound)
    assert torch.equal(c1, c2)   # the image form computes the same context, bit for bit
