"""Per-element reference tests of the cross-entropy kernels (csrc/ce.hip), of klab_gelu_fwd[_q8] (csrc/misc.hip) and of the gated-GELU gate
(csrc/ffn_gated.hip) against fp64 (references and bounds: tests/rowops_ref.py).

rule                                                                   -> shape
  ce: bf16 one-pass NIT = 8 up to V = 16384, NIT = 16 up to 32768,      -> V = 8 (three waves hold nothing), 2056, 16384 | 16392, 32768 | 32776, 40000
      two-pass above; f32 always two-pass, 1024 columns a sweep        -> V = 4, 1028, 4104
  ce: the label's lane subtracts 1                                     -> labels at column 0, V - 1, V - 3 (last vector), the middle, -100
  ce: row stride ld > V                                                -> ld = V + 16 with sentinels behind every row
  ce_count / ce_reduce: 256 threads stride over the rows               -> rows = 6 and 261
  gelu_poly (bf16), gelu_new through __expf (bf16)                     -> all 65280 finite bf16 values as a 16 x 4080 matrix
  stream_grid: second lap after 2048 * 256 vectors                     -> n = 2048 * 256 * 8 + 40 (bf16), * 4 + 40 (f32); M = 2050, F = 2056
  geglu row strides                                                    -> M = 37, F = 192, ldab = 2F + 64, ldh = F + 8, lddab = 2F + 8"""
import pytest
import torch

from tests import rowops_ref as R
from tests.rowops_ref import U8, U24, Guarded, assert_equal, assert_within

pytestmark = pytest.mark.gpu

SEED, BF16, F32 = 977, torch.bfloat16, torch.float32
LAP = 2048 * 256


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


@pytest.fixture(scope="module")
def seed():
    return torch.tensor([SEED], dtype=torch.int32).cuda()


# ---------------------------------------------------------------------------------------------------------------- cross-entropy
CE_CASES = [(6, V, dt) for dt in ("bf16", "f32") for V in R.CE_V[dt]] + [(261, 2056, "bf16"), (261, 1028, "f32")]


def _ce_run(ops, c, V, write_grad, count_first=False):
    rows = c["stored"].shape[0]
    ld = V + R.CE_PAD
    image = torch.full((rows, ld), R.CE_SENT, dtype=c["dtype"])
    image[:, :V] = c["stored"]
    buf = Guarded((rows, ld), c["dtype"], init=image)
    inv_n, loss_row, loss = Guarded((1,), F32), Guarded((rows,), F32), Guarded((1,), F32)
    labels = c["labels"].cuda()
    if count_first:
        ops.ce_count(labels, inv_n.t)
    ops.ce_fwd(buf.t[:, :V], labels, inv_n.t, loss_row.t, loss.t, write_grad=write_grad)
    return dict(image=image, logits=buf.check("logits"), inv_n=inv_n.check("inv_n"), loss_row=loss_row.check("loss_row"), loss=loss.check("loss"))


@pytest.mark.parametrize("rows,V,dt", CE_CASES)
def test_ce_fwd(ops, rows, V, dt):
    c = R.ce_case(rows, V, dt)
    tag = f" rows={rows} V={V} {dt}"
    # loss only: every byte of the logits survives
    a = _ce_run(ops, c, V, write_grad=False)
    assert_equal("ce_fwd logits (write_grad = False)", a["logits"], a["image"], tag)
    assert_equal("ce_fwd inv_n", a["inv_n"], c["inv_n"].reshape(1), tag)
    assert_within("ce_fwd loss_row", a["loss_row"], c["loss_row"], c["row_bound"], tag)
    assert bool((a["loss_row"][~c["valid"]] == 0).all()), f"ce_fwd loss_row{tag}: an ignored row has a loss"
    assert_within("ce_fwd loss", a["loss"], c["loss"].reshape(1), c["loss_bound"].reshape(1), tag)
    # with the gradient written in place
    b = _ce_run(ops, c, V, write_grad=True)
    assert_equal("ce_fwd sentinel columns behind V", b["logits"][:, V:], a["image"][:, V:], tag)
    grad = b["logits"][:, :V]
    assert bool((grad[~c["valid"]] == 0).all()), f"ce_fwd gradient{tag}: an ignored row has a gradient"
    assert_within("ce_fwd gradient", grad, c["grad"], c["gbound"], tag)
    assert_equal("ce_fwd loss_row (with gradient)", b["loss_row"], a["loss_row"], tag)
    assert_equal("ce_fwd loss (with gradient)", b["loss"], a["loss"], tag)
    # inv_n counted ahead of the logits: bit-identical
    d = _ce_run(ops, c, V, write_grad=3, count_first=True)
    for k in ("logits", "inv_n", "loss_row", "loss"):
        assert_equal(f"ce_fwd {k} (write_grad | 2 after ce_count)", d[k], b[k], tag)


# ---------------------------------------------------------------------------------------------------------------- GELU: all bf16 values
def test_gelu_fwd_every_finite_bf16(ops):
    x = R.all_finite_bf16()
    ref = R.gelu_erf64(x)
    y = Guarded((16, 4080), BF16)
    ops.gelu_fwd(x.cuda(), y.t)
    got = y.check("a")
    assert not bool(torch.isnan(got.float()).any()), "gelu_fwd: NaN for a finite input"
    assert_within("gelu_fwd a (bf16, every finite value)", got, ref, 1.2e-4 + U8 * ref.abs())
    # the fp8 form: the same bf16 image bit for bit, bytes and scales of that image
    y2, y8, ys = Guarded((16, 4080), BF16), Guarded((16, 4080), torch.uint8), Guarded((16,), F32)
    ops.gelu_fwd_q8(x.cuda(), y2.t, y8.t, ys.t)
    assert_equal("gelu_fwd_q8 a", y2.check("a").view(torch.int16), got.view(torch.int16))
    b, sc = R.q8_expected(got)
    assert_equal("gelu_fwd_q8 ascale", ys.check("ascale"), sc)
    assert_equal("gelu_fwd_q8 a8", R.unsigned_zero(y8.check("a8")), R.unsigned_zero(b))


def test_geglu_every_finite_bf16(ops):
    # b = 1 and dh = 1: h and db are gelu_new(a), da is its derivative
    a = R.all_finite_bf16()
    ab = torch.cat([a, torch.ones_like(a)], 1).cuda()
    ref, dref = R.gelu_new64(a)
    one = torch.ones(16, 4080, dtype=torch.float64)
    h = Guarded((16, 4080), BF16)
    ops.geglu_fwd(ab, h.t)
    got = h.check("h")
    assert not bool(torch.isnan(got.float()).any()), "geglu_fwd: NaN for a finite input"
    assert_within("geglu_fwd h (bf16, every finite value)", got, ref, R.gelu_new_bf16_bound(a, one, ref))
    dab = Guarded((16, 2 * 4080), BF16)
    ops.geglu_bwd(torch.ones(16, 4080, dtype=BF16).cuda(), ab, dab.t)
    gd = dab.check("dab")
    da, db = gd[:, :4080], gd[:, 4080:]
    bad = torch.isnan(da.float())
    assert not bool(bad.any()), f"geglu_bwd da: NaN for {int(bad.sum())} finite inputs, the smallest in size {float(a[bad].float().abs().min()):.3e}"
    assert not bool(torch.isnan(db.float()).any()), "geglu_bwd db: NaN for a finite input"
    assert_within("geglu_bwd db (bf16, every finite value)", db, ref, R.gelu_new_bf16_bound(a, one, ref))
    assert_within("geglu_bwd da (bf16, every finite value)", da, dref, R.gelu_new_grad_bf16_bound(a, one, dref))


# ---------------------------------------------------------------------------------------------------------------- f32 forms
def _f32_points():
    g = R.gen(9100)
    return torch.cat([3.0 * torch.randn(4096, generator=g), torch.tensor([0.0, -0.0, 1e-30, -1e-30, 5.5, -5.5, 20.0, -20.0])])


def test_gelu_fwd_f32(ops):
    x = _f32_points()
    ref = R.gelu_erf64(x)
    stated, used = R.gelu_f32_bound(x, ref)
    y = Guarded((x.numel(),), F32)
    ops.gelu_fwd(x.cuda(), y.t)
    got = y.check("a")
    err = (got.double() - ref).abs()
    print(f"gelu_fwd f32: worst err / (bound without the cancellation term) {float((err / stated.clamp_min(1e-300)).max()):.3e}")
    assert_within("gelu_fwd a (f32)", got, ref, used)


def test_geglu_f32(ops):
    a = _f32_points()
    n = a.numel()
    ab = torch.cat([a, torch.ones(n)])[None].cuda()
    ref, dref = R.gelu_new64(a)
    stated, used = R.gelu_f32_bound(a, ref)
    h = Guarded((1, n), F32)
    ops.geglu_fwd(ab, h.t)
    got = h.check("h")[0]
    print(f"geglu_fwd f32: worst err / (bound without the cancellation term) {float(((got.double() - ref).abs() / stated.clamp_min(1e-300)).max()):.3e}")
    assert_within("geglu_fwd h (f32)", got, ref, used)
    dab = Guarded((1, 2 * n), F32)
    ops.geglu_bwd(torch.ones(1, n).cuda(), ab, dab.t)
    gd = dab.check("dab")[0]
    assert_within("geglu_bwd db (f32)", gd[n:], ref, used)
    assert_within("geglu_bwd da (f32)", gd[:n], dref, R.gelu_new_grad_f32_bound(a, dref))


# ---------------------------------------------------------------------------------------------------------------- second lap, strides, dropout
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_gelu_fwd_second_lap(ops, dt):
    dtype, n = (BF16, LAP * 8 + 40) if dt == "bf16" else (F32, LAP * 4 + 40)
    g = R.gen(9200)
    x = (2.0 * torch.randn(n, generator=g)).to(dtype)
    ref = R.gelu_erf64(x)
    y = Guarded((n,), dtype)
    ops.gelu_fwd(x.cuda(), y.t)
    bound = 1.2e-4 + U8 * ref.abs() if dt == "bf16" else R.gelu_f32_bound(x, ref)[1]
    assert_within(f"gelu_fwd a ({dt}, n = {n})", y.check("a"), ref, bound)


def _geglu_case(ops, seed, M, F, dtype, ldab, ldh, lddab, p, tagn):
    g = R.gen(9300 + M + F)
    a = torch.randn(M, F, generator=g).to(dtype) * 2
    b = torch.randn(M, F, generator=g).to(dtype)
    dh = torch.randn(M, F, generator=g).to(dtype)
    # no operand may be zero where the mask is read off the output
    b[b == 0] = 1
    dh[dh == 0] = 1
    SENT = 55.0
    ab_img = torch.full((M, ldab), SENT, dtype=dtype)
    ab_img[:, :F], ab_img[:, F:2 * F] = a, b
    ab = ab_img.cuda()
    m = R.mask(SEED, tagn, p, R.remap_rows(M), F).double() if p else torch.ones(M, F, dtype=torch.float64)
    ga, dga = R.gelu_new64(a)
    tag = f" M={M} F={F} {dtype} p={p}"
    if dtype == BF16:
        val = lambda scale: R.gelu_new_bf16_bound(a, scale, ga * scale)            # scale >= 0: |ref| = |ga| scale
        der = lambda scale: R.gelu_new_grad_bf16_bound(a, scale, dga * scale)
    else:
        val = lambda scale: (R.gelu_f32_bound(a, ga)[1] + 4 * U24 * ga.abs()) * scale  # (three more f32 multiplications)
        der = lambda scale: (R.gelu_new_grad_f32_bound(a, dga) + 4 * U24 * dga.abs()) * scale
    h_img = torch.full((M, ldh), SENT, dtype=dtype)
    h = Guarded((M, ldh), dtype, init=h_img)
    ops.geglu_fwd(ab[:, :2 * F], h.t[:, :F], drop_p=p, seed_dev=seed if p else None, tag=tagn)
    got = h.check("h")
    assert_equal("geglu_fwd gap behind h", got[:, F:], h_img[:, F:], tag)
    live = ga.abs() > 1e-3  # (below a = -5.1 the bf16 tanh is -1 and the kernel's zero is no dropped element)
    if p:
        assert_equal("geglu_fwd mask (index m * F + f)", (got[:, :F].float() != 0) & live, (m != 0) & live, tag)
    assert_within("geglu_fwd h", got[:, :F], ga * b.double() * m, val(b.double().abs() * m), tag)
    dab_img = torch.full((M, lddab), SENT, dtype=dtype)
    dab = Guarded((M, lddab), dtype, init=dab_img)
    ops.geglu_bwd(dh.cuda(), ab[:, :2 * F], dab.t[:, :2 * F], drop_p=p, seed_dev=seed if p else None, tag=tagn)
    gd = dab.check("dab")
    assert_equal("geglu_bwd gap behind dab", gd[:, 2 * F:], dab_img[:, 2 * F:], tag)
    gm = dh.double() * m
    if p:
        assert_equal("geglu_bwd mask (index m * F + f)", (gd[:, F:2 * F].float() != 0) & live, (m != 0) & live, tag)
    assert_within("geglu_bwd db", gd[:, F:2 * F], gm * ga, val(gm.abs()), tag)
    assert_within("geglu_bwd da", gd[:, :F], gm * b.double() * dga, der((gm * b.double()).abs()), tag)
    assert_equal("geglu: ab untouched", ab.cpu(), ab_img, tag)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_geglu_row_strides_and_dropout(ops, seed, dt, p):
    F = 192
    _geglu_case(ops, seed, 37, F, BF16 if dt == "bf16" else F32, 2 * F + 64, F + 8, 2 * F + 8, p, 41)


def test_geglu_second_lap_with_dropout(ops, seed):
    M, F = 2050, 2056
    assert M * (F // 8) > LAP
    _geglu_case(ops, seed, M, F, BF16, 2 * F, F, 2 * F, 0.5, 42)
