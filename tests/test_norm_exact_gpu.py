"""Exact and per-element reference tests of csrc/norm.hip (references, fixtures and bounds: tests/rowops_ref.py).

rule of the dispatch                                             -> smallest shape that can break it
  RMS forward: 4 columns per lane, 256 per sweep                 -> d = 4 (one lane), 132 (ragged sweep), 256, 260 (second sweep), 1028
  one wave per row, 4 rows per workgroup, 2048 workgroups        -> rows = 1, 5 (second workgroup), 8197 (second lap)
  rmsnorm_fwd_q8: SLOTS = 1 / 2 / 4 at d <= 256 / 512 / 1024      -> d = 8, 132, 256 | 260, 512 | 516, 1024; 1028 is refused
  RMS backward fused: the same SLOTS, 16 waves, 512 workgroups   -> d = 12 .. 1024, rows = 1, 17 (second workgroup), 8200 (second lap)
  RMS backward split (dw absent, or d > 1024)                    -> d = 132 without dw; d = 1028, rows = 300 with dw
  LayerNorm forward: 4 rows per wave at C <= 64                  -> C = 4, 16, 64; rows = 1, 3, 5 (partly filled waves), 32771 (second lap)
                     2 rows per wave at C <= 128                 -> C = 68, 96, 128; rows = 1, 3, 16387
                     1 row per wave above                        -> C = 132, 256, 260, 1536; rows = 5, 8197
  LayerNorm backward fused (dy and a column sum, C <= 1024)      -> C = 16 .. 1024, rows = 1, 17, 8200
  LayerNorm backward split                                       -> dy alone; dgamma + dbeta alone; C = 1028 f32 / 1032 bf16 with dprev
                                                                    (colsum_kernel / colsum8_kernel)
Every output lies between guard bands, overwritten outputs start as NaN, accumulated ones from nonzero integers; every dropout
site is compared with rowops_ref.drop_mult at the element index its comment documents, once through a row remap."""
import pytest
import torch

from tests import rowops_ref as R
from tests.rowops_ref import U8, U24, Guarded, assert_equal, assert_within

pytestmark = pytest.mark.gpu

SEED, BF16, F32 = 1234, torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


@pytest.fixture(scope="module")
def seed():
    return torch.tensor([SEED], dtype=torch.int32).cuda()


def cu(t, dtype=F32):
    return t.to(dtype).cuda().contiguous()


def kept(name, got, m, extra=""):
    """the mask of an output whose operands are non-zero: a zero is a dropped element"""
    assert_equal(name + " mask", got.cpu().float() != 0, m != 0, extra)


# ---------------------------------------------------------------------------------------------------------------- RMS forward
@pytest.mark.parametrize("rows,d", R.RMS_FWD)
def test_rmsnorm_fwd(ops, seed, rows, d):
    fx = R.rms_randn(rows, d)
    x, w = cu(fx["x"]), cu(fx["w"])
    tag = f" rows={rows} d={d}"
    # (1) bf16 y, y_f32 and rstd, no dropout
    y, y32, rs = Guarded((rows, d), BF16), Guarded((rows, d), F32), Guarded((rows,), F32)
    ops.rmsnorm_fwd(x, w, y=y.t, y_f32=y32.t, rstd=rs.t)
    r_k = rs.check("rstd")
    assert_within("rmsnorm_fwd rstd", r_k, fx["r"], (R.adds(d) + 8) * U24 * fx["r"], tag)
    want = R.rms_fwd_from_stat(fx["x"], fx["w"], r_k)
    assert_equal("rmsnorm_fwd y_f32", y32.check("y_f32"), want, tag)
    assert_equal("rmsnorm_fwd y (bf16)", y.check("y"), want.to(BF16), tag)
    assert_within("rmsnorm_fwd y_f32 end to end", y32.t, fx["y"], (R.adds(d) + 12) * U24 * fx["y"].abs(), tag)
    assert_within("rmsnorm_fwd y (bf16) end to end", y.t, fx["y"], ((R.adds(d) + 12) * U24 + U8) * fx["y"].abs(), tag)
    # (2) f32 y alone, no rstd, dropout p = 0.5 at index row * d + c
    m = R.mask(SEED, 3, 0.5, R.remap_rows(rows), d)
    y = Guarded((rows, d), F32)
    ops.rmsnorm_fwd(x, w, y=y.t, drop_p=0.5, seed=seed, tag=3)
    got = y.check("y")
    kept("rmsnorm_fwd y (f32, dropout)", got, m, tag)
    assert_equal("rmsnorm_fwd y (f32, dropout)", got, R.rms_fwd_from_stat(fx["x"], fx["w"], r_k, m), tag)
    # (3) y_f32 alone through the row remap, dropout p = 0.25 at index orow * d + c; rows nobody owns stay NaN
    orow, total = R.remap_rows(rows, **R.REMAP), R.out_rows(rows, **R.REMAP)
    m = R.mask(SEED, 4, 0.25, orow, d)
    y32 = Guarded((total, d), F32)
    ops.rmsnorm_fwd(x, w, y_f32=y32.t, drop_p=0.25, seed=seed, tag=4, **R.REMAP)
    got = y32.check("y_f32")
    kept("rmsnorm_fwd y_f32 (remap, dropout)", got[orow], m, tag)
    assert_equal("rmsnorm_fwd y_f32 (remap, dropout)", got, R.scatter_rows(orow, R.rms_fwd_from_stat(fx["x"], fx["w"], r_k, m), total), tag)
    # (4) bf16 y through the remap, dropout (the second DROP = true instantiation) and without
    for p in (0.5, 0.0):
        m = R.mask(SEED, 5, p, orow, d) if p else None
        y = Guarded((total, d), BF16)
        ops.rmsnorm_fwd(x, w, y=y.t, drop_p=p, seed=seed, tag=5, **R.REMAP)
        assert_equal(f"rmsnorm_fwd y (bf16, remap, p={p})", y.check("y"),
                     R.scatter_rows(orow, R.rms_fwd_from_stat(fx["x"], fx["w"], r_k, m).to(BF16), total), tag)


@pytest.mark.parametrize("rows,d", R.RMS_Q8)
def test_rmsnorm_fwd_q8(ops, seed, rows, d):
    fx = R.rms_randn(rows, d, seed=1)
    xc = fx["x"].clone()
    xc[rows // 2] = 0.0  # one all-zero row: scale 1, bytes 0
    x, w = cu(xc), cu(fx["w"])
    tag = f" rows={rows} d={d}"
    r64 = (xc.double().pow(2).mean(-1) + 1e-6).rsqrt()
    for p in (0.0, 0.5):
        m = R.mask(SEED, 6, p, R.remap_rows(rows), d) if p else None
        y, rs, y8, ys = Guarded((rows, d), BF16), Guarded((rows,), F32), Guarded((rows, d), torch.uint8), Guarded((rows,), F32)
        if p:
            ops.rmsnorm_fwd_q8(x, w, y.t, rs.t, y8.t, ys.t, drop_p=p, seed=seed, tag=6)
        else:
            ops.rmsnorm_fwd_q8(x, w, y.t, rs.t, y8.t, ys.t)
        r_k = rs.check("rstd")
        assert_within(f"rmsnorm_fwd_q8 rstd p={p}", r_k, r64, (R.adds(d) + 8) * U24 * r64, tag)
        want = R.rms_fwd_from_stat(xc, fx["w"], r_k, m).to(BF16)
        got = y.check("y")
        if p:
            live = torch.arange(rows) != rows // 2
            kept("rmsnorm_fwd_q8 y", got[live], m[live], tag)
        assert_equal(f"rmsnorm_fwd_q8 y p={p}", got, want, tag)
        b, sc = R.q8_expected(want)
        assert_equal(f"rmsnorm_fwd_q8 yscale p={p}", ys.check("yscale"), sc, tag)
        assert float(sc[rows // 2]) == 1.0
        assert_equal(f"rmsnorm_fwd_q8 y8 p={p}", R.unsigned_zero(y8.check("y8")), R.unsigned_zero(b), tag)


def test_rmsnorm_fwd_q8_refuses_rows_wider_than_1024(ops):
    x, w = torch.ones(2, 1028).cuda(), torch.ones(1028).cuda()
    with pytest.raises(Exception):
        ops.rmsnorm_fwd_q8(x, w, torch.empty(2, 1028, dtype=BF16).cuda(), torch.empty(2).cuda(), torch.empty(2, 1028, dtype=torch.uint8).cuda(),
                           torch.empty(2).cuda())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- RMS backward
def _rms_bwd_inputs(fx, total=None, orow=None):
    dy = fx["dy"].float()
    if orow is not None:  # dy lives in the remapped row space; rows nobody owns hold NaN, which must never be read into a result
        dy = R.scatter_rows(orow, dy, total)
    return cu(dy), cu(fx["x"]), cu(fx["w"]), cu(fx["rstd"]), cu(fx["dres"])


def _rms_bwd_check(ops, seed, fx, rows, d, *, remap, dxt_dtype, want_dx, want_dxt, use_dres, dw_mode, tag):
    """one call of rmsnorm_bwd / rmsnorm_bwd_part on the exact fixture with p_y = p_prev = 0.5, everything torch.equal"""
    kw = R.REMAP if remap else {}
    orow = R.remap_rows(rows, **kw)
    total = R.out_rows(rows, **kw)
    my, mp = R.mask(SEED, 7, 0.5, orow, d), R.mask(SEED, 8, 0.5, R.remap_rows(rows), d)
    e = R.rms_bwd_exact(fx, my, mp, use_dres)
    dy, x, w, rstd, dres = _rms_bwd_inputs(fx, total, orow)
    dx = Guarded((rows, d), F32) if want_dx else None
    dxt = Guarded((rows, d), dxt_dtype) if want_dxt else None
    args = dict(dres=dres if use_dres else None, dx=dx.t if dx else None, dxt=dxt.t if dxt else None, p_y=0.5, tag_y=7, p_prev=0.5, tag_prev=8,
                seed=seed, **kw)
    if dw_mode == "part":
        nb = ops.rmsnorm_part_rows(rows)
        part = Guarded((nb + 1, d), F32)  # one guard row inside the NaN-filled buffer as well
        ops.rmsnorm_bwd_part(dy, x, w, rstd, part.t[:nb], **args)
        got = part.check("dw_part")
        assert bool(torch.isnan(got[nb]).all()), f"rmsnorm_bwd_part{tag}: the row behind the partials was written"
        assert not bool(torch.isnan(got[:nb]).any()), f"rmsnorm_bwd_part{tag}: a partial row was left unwritten"
        assert_equal("rmsnorm_bwd_part column sums of the partials", got[:nb].double().sum(0), e["dwsum"], tag)
    elif dw_mode == "dw":
        dw = Guarded((d,), F32, init=fx["dw0"].float())
        ops.rmsnorm_bwd(dy, x, w, rstd, dw=dw.t, **args)
        assert_equal("rmsnorm_bwd dw", dw.check("dw").double(), fx["dw0"] + e["dwsum"], tag)
    else:
        ops.rmsnorm_bwd(dy, x, w, rstd, **args)
    if dx:
        assert_equal("rmsnorm_bwd dx", dx.check("dx"), e["dx"], tag)
    if dxt:
        got = dxt.check("dxt")
        nz = e["dx"] != 0
        assert_equal("rmsnorm_bwd dxt mask (p_prev, index row * d + c)", (got.float() != 0) & nz, (mp != 0) & nz, tag)
        assert_equal(f"rmsnorm_bwd dxt ({dxt_dtype})", got, e["dxt32"].to(dxt_dtype), tag)


@pytest.mark.parametrize("rows,d", R.RMS_BWD)
def test_rmsnorm_bwd_fused_exact(ops, seed, rows, d):
    fx = R.rms_bwd_fixture(rows, d)
    tag = f" rows={rows} d={d}"
    c = lambda **k: _rms_bwd_check(ops, seed, fx, rows, d, tag=tag + f" {k}", **k)
    c(remap=False, dxt_dtype=BF16, want_dx=True, want_dxt=True, use_dres=True, dw_mode="dw")
    c(remap=True, dxt_dtype=F32, want_dx=False, want_dxt=True, use_dres=False, dw_mode="dw")
    c(remap=False, dxt_dtype=BF16, want_dx=True, want_dxt=False, use_dres=True, dw_mode="dw")
    c(remap=True, dxt_dtype=BF16, want_dx=True, want_dxt=True, use_dres=True, dw_mode="part")
    c(remap=False, dxt_dtype=F32, want_dx=True, want_dxt=True, use_dres=False, dw_mode="part")


@pytest.mark.parametrize("rows,d,with_dw", R.RMS_BWD_SPLIT)
def test_rmsnorm_bwd_split_exact(ops, seed, rows, d, with_dw):
    # dw absent (any d) or d > 1024: rmsnorm_bwd_kernel, and rmsnorm_dw_kernel for the weight gradient
    fx = R.rms_bwd_fixture(rows, d)
    tag = f" rows={rows} d={d}"
    mode = "dw" if with_dw else "none"
    c = lambda **k: _rms_bwd_check(ops, seed, fx, rows, d, tag=tag + f" {k}", dw_mode=mode, **k)
    c(remap=False, dxt_dtype=BF16, want_dx=True, want_dxt=True, use_dres=True)
    c(remap=True, dxt_dtype=F32, want_dx=True, want_dxt=True, use_dres=False)
    c(remap=True, dxt_dtype=BF16, want_dx=False, want_dxt=True, use_dres=True)


@pytest.mark.parametrize("rows,d", [(17, 132), (33, 516), (300, 1028)])
def test_rmsnorm_bwd_randn_per_element(ops, seed, rows, d):
    fx = R.rms_randn(rows, d, seed=2)
    g = R.gen(7400 + d)
    dyc, dresc = torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g)
    rk = fx["r"].float()
    my = R.mask(SEED, 9, 0.5, R.remap_rows(rows), d)
    ref = R.rms_bwd_reference(fx["x"], fx["w"], dyc, rk, dresc, my)
    dx, dxt, dw = Guarded((rows, d), F32), Guarded((rows, d), BF16), Guarded((d,), F32, init=torch.zeros(d))
    ops.rmsnorm_bwd(cu(dyc), cu(fx["x"]), cu(fx["w"]), cu(rk), dres=cu(dresc), dx=dx.t, dxt=dxt.t, dw=dw.t, p_y=0.5, tag_y=9, seed=seed)
    tag = f" rows={rows} d={d}"
    assert_within("rmsnorm_bwd dx (randn)", dx.check("dx"), ref["dx"], ref["bound"], tag)
    assert_within("rmsnorm_bwd dxt (randn, bf16)", dxt.check("dxt"), ref["dx"], ref["bound"] + U8 * ref["dx"].abs(), tag)
    assert_within("rmsnorm_bwd dw (randn)", dw.check("dw"), ref["dw"], ref["dw_bound"], tag)


# ---------------------------------------------------------------------------------------------------------------- LayerNorm forward
def _ln_stats(fx, C, mean_k, r_k, key, tag):
    lanes = R.ln_lanes(C)
    n = R.adds(C, lanes)
    y = fx["y" + key].double()
    assert_within("layernorm_fwd rstd", r_k, fx["r" + key], (n + 8) * U24 * fx["r" + key], tag)
    if key == "i":
        want = y.sum(-1).float() / torch.tensor(float(C), dtype=F32)
        assert_equal("layernorm_fwd mean (integer rows)", mean_k, want, tag)
    else:
        assert_within("layernorm_fwd mean", mean_k, fx["mu"], n * U24 * y.abs().sum(-1) / C + U24 * fx["mu"].abs(), tag)


@pytest.mark.parametrize("rows,C", R.LN_FWD)
def test_layernorm_fwd(ops, seed, rows, C):
    fx = R.ln_randn(rows, C)
    gam, bet, sc = fx["gamma"], fx["beta"], fx["shortcut"]
    g_d, b_d, s_d = cu(gam), cu(bet), cu(sc)
    tag = f" rows={rows} C={C}"
    orow, total = R.remap_rows(rows, **R.REMAP), R.out_rows(rows, **R.REMAP)
    # (1) f32 in, bf16 out: every output, shortcut, no dropout; statistics against fp64
    out, outt, mean, rstd = Guarded((rows, C), F32), Guarded((rows, C), BF16), Guarded((rows,), F32), Guarded((rows,), F32)
    ops.layernorm_fwd(cu(fx["y"]), g_d, b_d, shortcut=s_d, out=out.t, outt=outt.t, mean=mean.t, rstd=rstd.t)
    mu_k, r_k = mean.check("mean"), rstd.check("rstd")
    _ln_stats(fx, C, mu_k, r_k, "", tag)
    want = R.ln_fwd_from_stat(fx["y"], mu_k, r_k, gam, bet, sc)
    assert_equal("layernorm_fwd out (f32 in)", out.check("out"), want, tag)
    assert_equal("layernorm_fwd outt (f32 in, bf16 out)", outt.check("outt"), want.to(BF16), tag)
    # (2) bf16 in, f32 out: outt alone, no statistics, no shortcut, dropout p = 0.5 through the remap at index orow * C + c
    m = R.mask(SEED, 10, 0.5, orow, C)
    outt = Guarded((total, C), F32)
    ops.layernorm_fwd(cu(fx["y"], BF16), g_d, b_d, outt=outt.t, drop_p=0.5, seed=seed, tag=10, **R.REMAP)
    got = outt.check("outt")
    want = R.ln_fwd_from_stat(fx["y"], mu_k, r_k, gam, bet, None, m)
    nz = R.ln_fwd_from_stat(fx["y"], mu_k, r_k, gam, bet, None) != 0
    assert_equal("layernorm_fwd outt mask (remap)", (got[orow] != 0) & nz, (m != 0) & nz, tag)
    assert_equal("layernorm_fwd outt (bf16 in, f32 out, remap, dropout)", got, R.scatter_rows(orow, want, total), tag)
    # (3) f32 in, f32 out: out alone through the remap, no dropout; integer rows: the mean is exact
    out, mean, rstd = Guarded((total, C), F32), Guarded((rows,), F32), Guarded((rows,), F32)
    ops.layernorm_fwd(cu(fx["yi"]), g_d, b_d, shortcut=s_d, out=out.t, mean=mean.t, rstd=rstd.t, **R.REMAP)
    mu_i, r_i = mean.check("mean"), rstd.check("rstd")
    _ln_stats(fx, C, mu_i, r_i, "i", tag + " integer rows")
    assert_equal("layernorm_fwd out (f32 in, remap)", out.check("out"),
                 R.scatter_rows(orow, R.ln_fwd_from_stat(fx["yi"], mu_i, r_i, gam, bet, sc), total), tag)
    # (4) bf16 in, bf16 out: out and outt, dropout without remap, no statistics
    m = R.mask(SEED, 11, 0.5, R.remap_rows(rows), C)
    out, outt = Guarded((rows, C), F32), Guarded((rows, C), BF16)
    ops.layernorm_fwd(cu(fx["y"], BF16), g_d, b_d, shortcut=s_d, out=out.t, outt=outt.t, drop_p=0.5, seed=seed, tag=11)
    want = R.ln_fwd_from_stat(fx["y"], mu_k, r_k, gam, bet, sc, m)
    got = out.check("out")
    kept("layernorm_fwd out", got, m, tag)  # (the shortcut makes an exact zero before the mask a 2^-24 event)
    assert_equal("layernorm_fwd out (bf16 in, dropout)", got, want, tag)
    assert_equal("layernorm_fwd outt (bf16 in, bf16 out, dropout)", outt.check("outt"), want.to(BF16), tag)
    # (5) randn gamma end to end against fp64
    ref, bound = R.ln_fwd_reference(fx["y"], fx["gamma2"], bet, sc, C)
    out, outt = Guarded((rows, C), F32), Guarded((rows, C), BF16)
    ops.layernorm_fwd(cu(fx["y"]), cu(fx["gamma2"]), b_d, shortcut=s_d, out=out.t, outt=outt.t)
    assert_within("layernorm_fwd out end to end", out.check("out"), ref, bound, tag)
    assert_within("layernorm_fwd outt (bf16) end to end", outt.check("outt"), ref, bound + U8 * ref.abs(), tag)


@pytest.mark.parametrize("rows,C", R.LN_Q8)
def test_layernorm_fwd_q8(ops, rows, C):
    fx = R.ln_randn(rows, C, seed=1)
    gam, bet, sc = fx["gamma"], fx["beta"], fx["shortcut"]
    tag = f" rows={rows} C={C}"
    out, outt, mean, rstd = Guarded((rows, C), F32), Guarded((rows, C), BF16), Guarded((rows,), F32), Guarded((rows,), F32)
    o8, osc = Guarded((rows, C), torch.uint8), Guarded((rows,), F32)
    ops.layernorm_fwd_q8(cu(fx["y"], BF16), cu(gam), cu(bet), cu(sc), out.t, outt.t, mean.t, rstd.t, o8.t, osc.t)
    mu_k, r_k = mean.check("mean"), rstd.check("rstd")
    _ln_stats(fx, C, mu_k, r_k, "", tag)
    want = R.ln_fwd_from_stat(fx["y"], mu_k, r_k, gam, bet, sc)
    assert_equal("layernorm_fwd_q8 out", out.check("out"), want, tag)
    assert_equal("layernorm_fwd_q8 outt", outt.check("outt"), want.to(BF16), tag)
    b, s = R.q8_expected(want.to(BF16))
    assert_equal("layernorm_fwd_q8 oscale", osc.check("oscale"), s, tag)
    assert_equal("layernorm_fwd_q8 o8", R.unsigned_zero(o8.check("o8")), R.unsigned_zero(b), tag)


# ---------------------------------------------------------------------------------------------------------------- LayerNorm backward
def _ln_bwd_check(ops, seed, fx, rows, C, *, dtype, remap, p, want, tag):
    """one call of layernorm_bwd on the exact fixture; want: subset of {"dy", "dgamma", "dbeta", "dprev"}"""
    kw = R.REMAP if remap else {}
    orow, total = R.remap_rows(rows, **kw), R.out_rows(rows, **kw)
    m = R.mask(SEED, 12, p, orow, C) if p else None
    e = R.ln_bwd_exact(fx, m)
    dout = fx["dout"].float()
    if remap:
        dout = R.scatter_rows(orow, dout, total)
    dy = Guarded((rows, C), dtype) if "dy" in want else None
    acc = {k: Guarded((C,), F32, init=fx[k + "0"].float()) for k in ("dgamma", "dbeta", "dprev") if k in want}
    ops.layernorm_bwd(cu(dout), cu(fx["y"], dtype), cu(fx["gamma"]), cu(fx["mean"]), cu(fx["rstd"]), dy=dy.t if dy else None,
                      dgamma=acc["dgamma"].t if "dgamma" in acc else None, dbeta=acc["dbeta"].t if "dbeta" in acc else None,
                      dprev_bias=acc["dprev"].t if "dprev" in acc else None, drop_p=p, seed=seed, tag=12, **kw)
    if dy:
        assert_equal(f"layernorm_bwd dy ({dtype})", dy.check("dy"), e["dy"].to(dtype), tag)
    for k in ("dgamma", "dbeta"):
        if k in acc:
            assert_equal(f"layernorm_bwd {k}", acc[k].check(k).double(), fx[k + "0"] + e[k], tag)
    if "dprev" in acc:
        # the fused kernel sums its f32 dy before the store, the split path (C > 1024) sums what it stored
        # and each of the at most ceil(rows / 16) atomic adds rounds at the size of dprev0 + the running sum
        src = e["dy"].double() if C <= 1024 else e["dy"].to(dtype).double()
        bound = 2 * rows * U24 * src.abs().sum(0) + -(-rows // 16) * U24 * (fx["dprev0"].abs() + src.abs().sum(0))
        assert_within("layernorm_bwd dprev_bias", acc["dprev"].check("dprev"), fx["dprev0"] + src.sum(0), bound, tag)


@pytest.mark.parametrize("rows,C", R.LN_BWD)
def test_layernorm_bwd_fused_exact(ops, seed, rows, C):
    fx = R.ln_bwd_fixture(rows, C)
    tag = f" rows={rows} C={C}"
    c = lambda **k: _ln_bwd_check(ops, seed, fx, rows, C, tag=tag + f" {k}", **k)
    c(dtype=BF16, remap=False, p=0.0, want=("dy", "dgamma"))
    c(dtype=F32, remap=False, p=0.5, want=("dy", "dbeta"))
    c(dtype=BF16, remap=True, p=0.5, want=("dy", "dprev"))
    c(dtype=F32, remap=True, p=0.0, want=("dy", "dgamma", "dbeta", "dprev"))
    c(dtype=BF16, remap=False, p=0.5, want=("dy", "dgamma", "dbeta", "dprev"))


def test_layernorm_bwd_dprev_is_exact_at_a_power_of_two_width(ops):
    rows, C = R.LN_DPREV_EXACT
    fx = R.ln_bwd_fixture(rows, C)
    e = R.ln_bwd_exact(fx)
    dy, dprev = Guarded((rows, C), F32), Guarded((C,), F32, init=fx["dprev0"].float())
    ops.layernorm_bwd(cu(fx["dout"]), cu(fx["y"]), cu(fx["gamma"]), cu(fx["mean"]), cu(fx["rstd"]), dy=dy.t, dprev_bias=dprev.t)
    assert_equal("layernorm_bwd dy", dy.check("dy"), e["dy"])
    assert_equal("layernorm_bwd dprev_bias (exact)", dprev.check("dprev").double(), fx["dprev0"] + e["dy"].double().sum(0))


@pytest.mark.parametrize("rows,C", R.LN_BWD_SUBSETS)
def test_layernorm_bwd_split_subsets_exact(ops, seed, rows, C):
    # dy alone: layernorm_bwd_kernel; dgamma / dbeta without dy: layernorm_dgb_kernel; both with dropout through the remap
    fx = R.ln_bwd_fixture(rows, C, seed=1)
    tag = f" rows={rows} C={C}"
    c = lambda **k: _ln_bwd_check(ops, seed, fx, rows, C, tag=tag + f" {k}", **k)
    c(dtype=BF16, remap=True, p=0.5, want=("dy",))
    c(dtype=F32, remap=False, p=0.0, want=("dy",))
    c(dtype=BF16, remap=True, p=0.5, want=("dgamma", "dbeta"))
    c(dtype=F32, remap=False, p=0.5, want=("dgamma",))
    c(dtype=F32, remap=False, p=0.0, want=("dbeta",))


@pytest.mark.parametrize("rows,C,dt", R.LN_BWD_SPLIT)
def test_layernorm_bwd_split_wide_rows_with_dprev(ops, seed, rows, C, dt):
    fx = R.ln_bwd_fixture(rows, C, seed=2)
    dtype = F32 if dt == "f32" else BF16
    tag = f" rows={rows} C={C} {dt}"
    _ln_bwd_check(ops, seed, fx, rows, C, dtype=dtype, remap=False, p=0.5, want=("dy", "dgamma", "dbeta", "dprev"), tag=tag)
    _ln_bwd_check(ops, seed, fx, rows, C, dtype=dtype, remap=True, p=0.0, want=("dy", "dprev"), tag=tag + " remap")


@pytest.mark.parametrize("rows,C,dt", [(17, 132, "f32"), (33, 516, "bf16"), (37, 1028, "bf16")])
def test_layernorm_bwd_randn_per_element(ops, seed, rows, C, dt):
    dtype = F32 if dt == "f32" else BF16
    fx = R.ln_randn(rows, C, seed=3)
    g = R.gen(7500 + C)
    dout = torch.randn(rows, C, generator=g)
    mean, rstd = fx["mu"].float(), fx["r"].float()
    m = R.mask(SEED, 13, 0.5, R.remap_rows(rows), C)
    ref = R.ln_bwd_reference(fx["y"], fx["gamma2"], mean, rstd, dout, m)
    dy, dg, db = Guarded((rows, C), dtype), Guarded((C,), F32, init=torch.zeros(C)), Guarded((C,), F32, init=torch.zeros(C))
    ops.layernorm_bwd(cu(dout), cu(fx["y"], dtype), cu(fx["gamma2"]), cu(mean), cu(rstd), dy=dy.t, dgamma=dg.t, dbeta=db.t, drop_p=0.5, seed=seed,
                      tag=13)
    tag = f" rows={rows} C={C} {dt}"
    assert_within("layernorm_bwd dy (randn)", dy.check("dy"), ref["dy"], ref["bound"] + (U8 * ref["dy"].abs() if dtype == BF16 else 0.0), tag)
    assert_within("layernorm_bwd dgamma (randn)", dg.check("dgamma"), ref["dgamma"], ref["dgamma_bound"], tag)
    assert_within("layernorm_bwd dbeta (randn)", db.check("dbeta"), ref["dbeta"], ref["dbeta_bound"], tag)
