"""decode_attn_kernel<T, DK, SLOT> (csrc/attn_t5.hip, klab_t5_beam_decode_attn, ops.decode_attn) against tests/decode_attn_ref.py: exact
fixtures (torch.equal), random operands inside a per-element bound derived from the formats, bit-reproducibility and the argument
checks.  tests/test_decode_attn_fixtures_cpu.py proves the fixtures, the layouts and the bound's sharpness (mutations) on the CPU.

rule (line of attn_t5.hip at this commit) -> shape
  for (j = lane; j < Lk; j += 64) (390)          Lk 1, 6: lanes without a key (m stays -inf, f = 0, 407); Lk 63 / 64 / 65: the last lane
                                                 empty, every lane one key, lane 0 alone on a second lap; Lk 130, 200: laps 3 and 4, ragged
  corr = __expf(m - mn), o * corr + pe * v (398-401)   chosen keys on lap 2 / 3 behind unchosen ones (corr = 0), on two laps of one lane
                                                 (corr = 1), on lap 1 with unchosen keys behind (pe = 0); random: every lane rescales
  SLOT ? kv_slot[b * slot_ld + j] : b / kv_group (385, 391)   slot-table form (a bijection of the rows per key, slot_ld = Lk + 3) and the
                                                 group form with kv_group 1 and 2 (R = 6 rows over 3 samples: the engine runs samples x group rows)
  srow * kv_bstride + j * ldk + h * DK (392-393)  self-attention layout (q | k | v interleaved, ldk = 3 inner, kv_bstride = cache rows x ldk)
                                                 and cross-attention layout (layer 1 of 3, ldk = 3 * 2 * inner, kv_bstride = Le * ldk)
  if (bias_row) s += bias_row[h * bias_ld + j] (397)   with and without; row t of an [H, Lt, Lt] table (bias_ld = Lt * Lt), pitch Lk + 5
  switch (dk) (432-439)                          dk 8, 16, 32, 64, 128 at Lk 65 and 200; dk 8 and 64 at every Lk; dk 24 refused
  orow = ctx + b * ctx_bstride + h * DK (412)    ctx_bstride = inner + 8 between guard bands, NaN before the launch
H = 3 (odd, so a head slip leaves the row), R = 5 (6 with kv_group 2).  NaN fills whatever must not be read: cache rows >= Lk, the q
blocks of other positions, the other layers' columns, bias columns >= Lk; slot entries at j >= Lk are valid slots whose rows are NaN.
No index of these tests leaves its buffer.

Out of scope: a bias of -inf or of float-min magnitude.  No caller passes one, and `m - mn` is NaN when a lane's first key is at
-inf (-inf - -inf), so the kernel has no defined result there."""
import pytest
import torch

from tests import decode_attn_ref as D
from tests import rowops_ref as RO

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "bf16")


def run(c, dtype, name="ctx"):
    """one launch on the layout of decode_attn_ref.layout; ctx rows of pitch inner + 8 between guard bands, all NaN before"""
    from klab_multimodalmodel_amd import ops
    q, k, v, kw, _ = D.layout(c, dtype, "cuda")
    inner = D.H * c.dk
    out = RO.Guarded((c.rows, inner + 8), dtype)
    ops.decode_attn(q, k, v, out.t, ctx_bstride=inner + 8, **kw)
    torch.cuda.synchronize()
    t = out.check(name)
    assert bool(torch.isnan(t[:, inner:]).all()), f"{name}: the columns between two rows were written"
    return t[:, :inner].reshape(c.rows, D.H, c.dk)


@pytest.mark.parametrize("form,g", D.FORMS)
@pytest.mark.parametrize("dn", DTYPES)
def test_decode_attn_is_exact_on_the_dyadic_fixtures(dn, form, g):
    """probabilities of exactly 1 / n on the chosen keys: the context is the mean of n values of V, bit for bit"""
    dtype = D.DT[dn]
    for Lk, dk in D.shapes():
        for wb in (True, False):
            f = D.exact_fixture(dn, form, g, Lk, dk, wb)
            got = run(f, dtype)
            RO.assert_equal(f"ctx {dn} {form} group {g} Lk {Lk} dk {dk} bias {wb}", got, f.want.to(dtype))


@pytest.mark.parametrize("form,g", D.FORMS)
@pytest.mark.parametrize("dn", DTYPES)
def test_decode_attn_random_operands_within_the_bound(dn, form, g):
    """every element inside decode_attn_ref.bound (scores up to about 60)"""
    dtype = D.DT[dn]
    worst = 0.0
    for _f, _g, Lk, dk, wb in [c for c in D.cases(random_only=True) if c[:2] == (form, g)]:
        c = D.random_case(dn, form, g, Lk, dk, wb)
        r = D.reference(c.q, c.K, c.V, c.bias, Lk, c.kv_slot, g)
        got = run(c, dtype)
        worst = max(worst, RO.assert_within(f"ctx {dn} {form} group {g} Lk {Lk} dk {dk} bias {wb}", got, r["ctx"], D.bound(r, Lk, dk, dtype)))
    print(f"decode_attn {dn} {form} group {g}: worst err / bound {worst:.3f}")


def test_decode_attn_is_bit_reproducible():
    """no atomics, a fixed merge order: two launches give the same bits"""
    for dn in DTYPES:
        c = D.random_case(dn, "slot", 1, 200, 64, True)
        a, b = run(c, D.DT[dn]), run(c, D.DT[dn])
        assert torch.equal(a.view(torch.int32 if dn == "f32" else torch.int16), b.view(torch.int32 if dn == "f32" else torch.int16))


def test_decode_attn_bad_arguments(monkeypatch):
    """ops.decode_attn raises before it calls the library, the entry point itself returns an error before any launch: ctx keeps its NaN"""
    from klab_multimodalmodel_amd import _lib as L
    from klab_multimodalmodel_amd import ops
    nh, dk, Lk, nrows = 2, 8, 4, 2
    inner = nh * dk
    q = torch.zeros(nrows, inner, device="cuda")
    kv = torch.zeros(nrows, Lk, 2 * inner, device="cuda")
    k, v = kv.view(-1), kv.view(-1)[inner:]
    slot = torch.zeros(nrows, Lk, dtype=torch.int32, device="cuda")
    ctx = torch.full((nrows, inner), float("nan"), device="cuda")
    ok = dict(R=nrows, H=nh, Lk=Lk, dk=dk, q_bstride=inner, kv_bstride=Lk * 2 * inner, ldk=2 * inner, ctx_bstride=inner)
    lib = L.load()
    called = []

    class Spy:  # the wrapper must not reach the library on any of these
        def __getattr__(self, name):
            called.append(name)
            return getattr(lib, name)

    with monkeypatch.context() as mp:
        mp.setattr(L, "load", lambda: Spy())
        with pytest.raises(NotImplementedError):
            ops.decode_attn(q, k, v, ctx, **{**ok, "dk": 24})
        for i in range(4):
            args = [q, k, v, ctx]
            args[i] = None
            with pytest.raises(ValueError):
                ops.decode_attn(*args, **ok)
        for bad in (dict(R=0), dict(R=-1), dict(kv_group=0), dict(kv_slot=slot, slot_ld=Lk - 1)):
            with pytest.raises(ValueError):
                ops.decode_attn(q, k, v, ctx, **{**ok, **bad})
        with pytest.raises(ValueError):
            ops.decode_attn(q.half(), k.half(), v.half(), ctx.half(), **ok)  # neither bf16 nor f32
        with pytest.raises(ValueError):
            ops.decode_attn(q, k.bfloat16(), v, ctx, **ok)  # two dtypes
        assert called == [], called

    def entry(dtype=L.F32, qp=q.data_ptr(), kp=k.data_ptr(), vp=v.data_ptr(), cp=ctx.data_ptr(), nr=nrows, group=1, sp=None, sld=0, d=dk):
        return lib.klab_t5_beam_decode_attn(dtype, qp, inner, kp, vp, Lk * 2 * inner, 2 * inner, group, sp, sld, None, 0, cp, inner, nr, nh,
                                            Lk, d, L.stream_ptr())

    assert entry(d=24) == L.ERR_UNSUPPORTED
    for bad in (dict(qp=None), dict(kp=None), dict(vp=None), dict(cp=None), dict(nr=0), dict(nr=-1), dict(group=0),
                dict(sp=slot.data_ptr(), sld=Lk - 1), dict(dtype=99)):
        assert entry(**bad) == L.ERR_BADARG, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(ctx).all())
    ops.decode_attn(q, k, v, ctx, kv_slot=slot, slot_ld=Lk, **ok)  # ... and the good call writes: zero scores, the mean of zeros
    torch.cuda.synchronize()
    assert bool((ctx == 0).all())
