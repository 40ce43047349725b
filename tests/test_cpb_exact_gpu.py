"""The Swin-V2 continuous-position-bias kernels against tests/cpb_ref.py: exact fixtures (torch.equal), real tables with random weights
inside per-element bounds derived from the formats, the add-to / overwrite contract of every output and the refusals.
tests/test_cpb_fixtures_cpu.py proves the fixtures and the bounds' sharpness (mutations) on the CPU.

rule (attn_swin.hip = S, attn_swin_large.hip = L, lines at this commit) -> shape
  forward
    __shared__ hid[512]; nhidden > 512 refused (S702, S1190, L631)       nh 512 fills it, nh 513 is refused by both entry points
    for (j = tid; j < nh; j += 256) (S706, S714)                          nh 40: most threads idle, one wave's worth of units; nh 300: a ragged
                                                                          second lap; nh 512: two full laps
    for (h = 0; h < H; ++h), red[4] (S712-720)                            H 1, 3, 32
    fmaxf(.., 0) (S707), if (hidden_out) (S709)                           pre-activations exactly 0 and negative; with and without hidden
    gather index[ij] * H + h (S726), sigmoid of the table form (L499)     w 2, 4, 7, 8 (n 4 .. 64, ntab 9 .. 225): dense == table form bit for bit
  backward
    if (!dtable_zeroed) memset (S1207-1210)                               NaN dtable with 0; cleared and preset dtable with 1
    atomicAdd(dtable + index[ij] * H + h, ..) (S738)                      real index (up to n entries per table row), synthetic index
    if (ntab > 192) any-size form (S1214)                                 ntab 192 (LDS form, all 12 register slots, last row in slot 12 of
                                                                          slice 15) and 193 (first size on the any-size kernel); 225: the default tower
    TI = 12, t = tt + i * 16 < ntab (S745, S756-757)                      ntab 9: slices 9..15 hold no row; 49; 169: eleven of twelve slots
    LDS size, max(H, 3) (S1216-1217, S787)                                H 1 (< 3); H 48 at ntab 169 refused (above 64 KiB)
    for (h = tt; h < H; h += 16) (S774)                                   H 24, 32: a second lap of the dW2 reduction; H 3, 4: idle slices
    j = blockIdx.x * 16 + tj < nh (S750-751)                              nh 40: the last block is half empty; nh 512
    hv > 0 gate (S785, L525)                                              a third of hidden exactly 0
    += into dW0, db0, dW2 (S778, S793, L534-537)                          initial contents 5, -3, 7
    any-size: s[CPB_MAXH], if (h < H), heads > 64 refused (L508-542, L615)  H 1, 8, 64; 65 refused by the any-size form and by the table form
    table form: dtable overwritten (L503)                                 NaN dtable
Every output lies between guard bands (rowops_ref.Guarded); overwritten ones start as NaN, accumulated ones from a non-zero integer."""
import pytest
import torch

from tests import cpb_ref as C
from tests import rowops_ref as RO

pytestmark = pytest.mark.gpu


def dev(t):
    return t.float().contiguous().cuda()


def idx(fx):
    return fx.index.to(torch.int32).contiguous().cuda()


def run_forward(fx, form, want_hidden):
    """form 'dense': klab_swin_cpb_bias -> table, bias [H, n * n], hidden; 'table': klab_swin_cpb_table -> table, btab [ntab, H], hidden"""
    from klab_multimodalmodel_amd import ops
    table = RO.Guarded((fx.ntab, fx.H), torch.float32)
    hidden = RO.Guarded((fx.ntab, fx.nh), torch.float32)
    out = RO.Guarded((fx.H, fx.n * fx.n) if form == "dense" else (fx.ntab, fx.H), torch.float32)
    if form == "dense":
        ops.swin_cpb_bias(dev(fx.coords), idx(fx), dev(fx.w0), dev(fx.b0), dev(fx.w2), table.t, out.t, hidden.t if want_hidden else None,
                          n=fx.n, heads=fx.H)
    else:
        ops.swin_cpb_table(dev(fx.coords), dev(fx.w0), dev(fx.b0), dev(fx.w2), table.t, out.t, hidden.t if want_hidden else None, heads=fx.H)
    torch.cuda.synchronize()
    h = hidden.check("hidden")
    assert want_hidden or bool(torch.isnan(h).all()), "hidden written without being asked for"
    return table.check("table"), out.check(form), h


@pytest.mark.parametrize("w", C.FWD_W)
def test_cpb_forward_is_exact_on_the_dyadic_fixture(w):
    """table and hidden bit for bit; the dense bias is the gather of the table form's bias table, bit for bit"""
    for H in C.FWD_H:
        for nh in C.FWD_NH:
            fx = C.fwd_exact_fixture(w, H, nh)
            what = f" w {w} H {H} nh {nh}"
            t_d, bias, h_d = run_forward(fx, "dense", True)
            t_t, btab, h_t = run_forward(fx, "table", True)
            t_d0, bias0, _ = run_forward(fx, "dense", False)
            t_t0, btab0, _ = run_forward(fx, "table", False)
            for name, t in (("table dense", t_d), ("table", t_t), ("table dense, no hidden", t_d0), ("table, no hidden", t_t0)):
                RO.assert_equal(name, t, fx.ref["table"].float(), what)
            for name, h in (("hidden dense", h_d), ("hidden", h_t)):
                RO.assert_equal(name, h, fx.ref["hidden"].float(), what)
            RO.assert_equal("bias against btab[index]", bias, C.dense(btab, fx.index, fx.n), what)
            RO.assert_equal("bias, no hidden", bias0, bias, what)
            RO.assert_equal("btab, no hidden", btab0, btab, what)


@pytest.mark.parametrize("w,pw", C.REAL_WINDOWS)
def test_cpb_forward_real_tables_within_the_bound(w, pw):
    worst = 0.0
    for H in C.FWD_H:
        for nh in C.FWD_NH:
            fx = C.fwd_random_fixture(w, pw, H, nh)
            what = f" w {w} pw {pw} H {H} nh {nh}"
            e_hid, e_tab, e_b = C.fwd_bounds(fx)
            t_d, bias, h_d = run_forward(fx, "dense", True)
            t_t, btab, h_t = run_forward(fx, "table", True)
            RO.assert_equal("table: dense against table form", t_d, t_t, what)
            RO.assert_equal("bias against btab[index]", bias, C.dense(btab, fx.index, fx.n), what)
            worst = max(worst, RO.assert_within("hidden", h_t, fx.ref["hidden"], e_hid, what), RO.assert_within("hidden dense", h_d, fx.ref["hidden"], e_hid, what),
                        RO.assert_within("table", t_t, fx.ref["table"], e_tab, what), RO.assert_within("btab", btab, fx.ref["btab"], e_b, what),
                        RO.assert_within("bias", bias, C.dense(fx.ref["btab"], fx.index, fx.n), C.dense(e_b, fx.index, fx.n), what))
    print(f"cpb forward w {w} pw {pw}: worst err / bound {worst:.3f}")


def test_cpb_forward_refuses_513_hidden_units():
    from klab_multimodalmodel_amd import ops
    fx = C.fwd_exact_fixture(2, 1, 40)
    w0, b0, w2 = torch.zeros(513, 2, device="cuda"), torch.zeros(513, device="cuda"), torch.zeros(1, 513, device="cuda")
    table, out, btab = (RO.Guarded(s, torch.float32) for s in ((fx.ntab, 1), (1, fx.n * fx.n), (fx.ntab, 1)))
    with pytest.raises(NotImplementedError):
        ops.swin_cpb_bias(dev(fx.coords), idx(fx), w0, b0, w2, table.t, out.t, None, n=fx.n, heads=1)
    with pytest.raises(NotImplementedError):
        ops.swin_cpb_table(dev(fx.coords), w0, b0, w2, table.t, btab.t, None, heads=1)
    torch.cuda.synchronize()
    for name, g in (("table", table), ("bias", out), ("btab", btab)):
        assert bool(torch.isnan(g.check(name)).all()), name


# ---- backward ----------------------------------------------------------------------------------------------------------------------
def _outputs(fx, dtable_init=None):
    d = dict(dtable=RO.Guarded((fx.ntab, fx.H), torch.float32, init=dtable_init),
             dw0=RO.Guarded((fx.nh, 2), torch.float32, init=torch.full((fx.nh, 2), fx.init["dw0"])),
             db0=RO.Guarded((fx.nh,), torch.float32, init=torch.full((fx.nh,), fx.init["db0"])),
             dw2=RO.Guarded((fx.H, fx.nh), torch.float32, init=torch.full((fx.H, fx.nh), fx.init["dw2"])))
    return d


def run_backward(fx, zeroed=False, dtable_init=None):
    """klab_swin_cpb_bias_bwd_pz; dtable starts as NaN unless dtable_init says otherwise"""
    from klab_multimodalmodel_amd import ops
    o = _outputs(fx, dtable_init)
    ops.swin_cpb_bias_bwd(dev(fx.dbias), dev(fx.bias), idx(fx), dev(fx.coords), dev(fx.hidden), dev(fx.w2), o["dtable"].t, o["dw0"].t, o["db0"].t,
                          o["dw2"].t, heads=fx.H, n=fx.n, ntab=fx.ntab, nhidden=fx.nh, dtable_zeroed=zeroed)
    torch.cuda.synchronize()
    return {k: g.check(k) for k, g in o.items()}


def run_table_backward(fx):
    from klab_multimodalmodel_amd import ops
    o = _outputs(fx)
    ops.swin_cpb_table_bwd(dev(fx.dbtab), dev(fx.btab), dev(fx.coords), dev(fx.hidden), dev(fx.w2), o["dtable"].t, o["dw0"].t, o["db0"].t,
                           o["dw2"].t, heads=fx.H)
    torch.cuda.synchronize()
    return {k: g.check(k) for k, g in o.items()}


@pytest.mark.parametrize("ntab,n,real", C.BWD_CASES)
def test_cpb_backward_is_exact_on_the_integer_fixture(ntab, n, real):
    """dtable, dW0, db0, dW2 = fp64 result + initial content, bit for bit, from the dense form (NaN dtable, dtable_zeroed = 0) and from
    the table form on the scattered gradient"""
    for case in C.bwd_exact_cases():
        if case[:3] != (ntab, n, real):
            continue
        fx = C.bwd_exact_fixture(*case)
        want = C.backward(fx)
        what = f" ntab {ntab} n {n} H {case[3]} nh {case[4]}"
        got = run_backward(fx)
        got_t = run_table_backward(fx)
        for k in C.OUTPUTS:
            RO.assert_equal(k, got[k], want[k].float(), what)
            RO.assert_equal(k + " (table form)", got_t[k], want[k].float(), what)


@pytest.mark.parametrize("case", [(169, 49, True, 3, 40), (169, 49, True, 24, 512), (225, 64, True, 8, 40), (193, 49, False, 64, 512)])
def test_cpb_backward_dtable_contract(case):
    """dtable_zeroed = 1 adds the scatter to what dtable holds: correct on a cleared buffer, c + gradient on one preset to c (the engine
    clears every block's slice in one fill and relies on this), and the MLP backward then runs on that sum"""
    fx = C.bwd_exact_fixture(*case)
    got = run_backward(fx, zeroed=True, dtable_init=torch.zeros(fx.ntab, fx.H))
    want = C.backward(fx)
    for k in C.OUTPUTS:
        RO.assert_equal(k + " cleared", got[k], want[k].float(), f" {case}")
    c = torch.full((fx.ntab, fx.H), 2.0)
    got = run_backward(fx, zeroed=True, dtable_init=c)
    want = C.backward(fx, dtable0=c.double())
    for k in C.OUTPUTS:
        RO.assert_equal(k + " preset 2", got[k], want[k].float(), f" {case}")
    got = run_backward(fx, zeroed=False, dtable_init=c)  # ... and dtable_zeroed = 0 clears it first
    want = C.backward(fx)
    for k in C.OUTPUTS:
        RO.assert_equal(k + " preset 2, not vouched for", got[k], want[k].float(), f" {case}")


def test_cpb_backward_refusals():
    """above 64 heads on the any-size form and the table form, above 64 KiB of LDS on the other: unsupported, and dW0, db0, dW2 keep their
    content (dtable is scratch: the dense form has scattered into it by then)"""
    from klab_multimodalmodel_amd import ops
    for ntab, n, real, H, table_form in ((193, 49, False, 65, False), (225, 64, True, 65, False), (225, 64, True, 65, True), (169, 49, True, 48, False)):
        base = C.bwd_exact_fixture(ntab, n, real, 1, 40)
        fx = C.Fx()
        fx.ntab, fx.n, fx.H, fx.nh, fx.index, fx.coords, fx.init = ntab, n, H, 40, base.index, base.coords, base.init
        fx.hidden, fx.w2 = base.hidden, torch.ones(H, 40, dtype=torch.float64)
        fx.btab = torch.full((ntab, H), 8.0, dtype=torch.float64)
        fx.bias, fx.dbias, fx.dbtab = C.dense(fx.btab, fx.index, n), torch.ones(H, n * n, dtype=torch.float64), torch.ones(ntab, H, dtype=torch.float64)
        o = _outputs(fx)
        with pytest.raises(NotImplementedError):
            if table_form:
                ops.swin_cpb_table_bwd(dev(fx.dbtab), dev(fx.btab), dev(fx.coords), dev(fx.hidden), dev(fx.w2), o["dtable"].t, o["dw0"].t,
                                       o["db0"].t, o["dw2"].t, heads=H)
            else:
                ops.swin_cpb_bias_bwd(dev(fx.dbias), dev(fx.bias), idx(fx), dev(fx.coords), dev(fx.hidden), dev(fx.w2), o["dtable"].t, o["dw0"].t,
                                      o["db0"].t, o["dw2"].t, heads=H, n=n, ntab=ntab, nhidden=40)
        torch.cuda.synchronize()
        for k in ("dw0", "db0", "dw2"):
            t = o[k].check(k)
            assert bool((t == fx.init[k]).all()), (ntab, H, table_form, k)
        o["dtable"].check("dtable")


@pytest.mark.parametrize("w,pw,H,nh", C.BWD_RANDOM)
def test_cpb_backward_real_tables_within_the_bound(w, pw, H, nh):
    """hidden and bias from the forward kernel, random dbias: every element of the four outputs inside cpb_ref.bwd_bounds"""
    f = C.fwd_random_fixture(w, pw, H, nh)
    _t, bias, hidden = run_forward(f, "dense", True)
    fx = C.bwd_random_fixture(w, pw, H, nh, hidden=hidden.double(), bias=bias.double())
    want = C.backward(fx)
    bounds = C.bwd_bounds(fx, want)
    got = run_backward(fx)
    worst = max(RO.assert_within(k, got[k], want[k], bounds[k], f" w {w} pw {pw} H {H} nh {nh}") for k in C.OUTPUTS)
    print(f"cpb backward w {w} pw {pw} H {H} nh {nh}: worst err / bound {worst:.3f}")
