"""klab_t5_attn_fwd / klab_t5_attn_bwd (and klab_dbias_reduce behind ds_defer) against exact references.

The fixtures of tests/exact_ref.py make every probability 0 or a power of two, so every output is a short sum of small dyadic
numbers that bf16 holds exactly (tests/test_exact_fixtures_cpu.py proves it in fp64).  Assertions:
  * whatever a kernel stores as bf16 (ctx, dq, dk, dv, the stored-dS slab): torch.equal with the fp64 reference cast to bf16 -- an
    f32 perturbation below 2^-9 relative vanishes in the store, exact zeros stay zero;
  * f32 outputs (lse, dbias, everything the f32 kernel writes): |got - ref| <= 2^-20 |ref| per element (one exp, one log and a
    reciprocal at a few f32 ulp each; 2^-20 is 16 ulp), and exactly 0 where the reference is 0.  Where the output is a sum
    (dbias over the batch, the f32 kernel's dq / dk / dv) |ref| is replaced by the sum of the magnitudes of its terms, because
    terms perturbed in f32 need not cancel the way the exact ones do; a sum whose terms are all 0 must still be exactly 0.
  * every output sits in a sentinel-filled buffer with leading dimensions larger than H dk (k | v, ctx | dO and dk | dv share
    fused buffers, as in the engine) and guard rows before and after; everything outside the written region must be unchanged.
A wrong last query row of a ragged tile, a key block skipped or added twice, a wrong head or key index in one workgroup or a
mis-masked edge fragment changes some element by at least its last bit and fails; the message names the first such element.

The one-workgroup kernels run once more under dropout at p = 0.5 against exact_ref.attn_drop_mult, the mask stated on its own.  The
harness (sentinel buffers, the comparisons) lives in tests/attn_harness.py, shared with tests/test_attn_fused_exact_gpu.py.

The last section runs each kernel family once on randn operands under per-element bounds counted from the roundings on each
output's data path (exact_ref.attn_fwd_bound, attn_bwd_bounds, attn_f32_bounds; DESIGN.md section 1 has the derivation and the
measured worst ratios)."""
import pytest
import torch

from tests import exact_ref as R
from tests.attn_harness import (GUARD, FlatOut, MatOut, assert_bf16_equal, assert_f32_close, first_bad, fused_input, ratio)

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
B, H = R.ATTN_B, R.ATTN_H


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


def assert_out(got, ref, what, mag=None):
    if got.dtype == torch.bfloat16:
        assert_bf16_equal(got, ref, what)
    else:
        assert_f32_close(got, ref, what, mag)


class Problem:
    """device operands of one attention problem in the engine's buffer layout: q alone, k | v fused, ctx | dO fused"""

    def __init__(self, q, k, v, do, bias, dtype, Lq, Lk, dk, causal, drop=None):
        self.Lq, self.Lk, self.dk, self.causal, self.dtype = Lq, Lk, dk, causal, dtype
        self.nb = q.shape[0]
        self.qbuf, self.ldq, (self.q,) = fused_input([q], dtype)
        self.kvbuf, self.ldkv, (self.k, self.v) = fused_input([k, v], dtype)
        self.do = do
        self.bias = None if bias is None else bias.float().cuda()
        self.kw = dict(B=self.nb, H=H, Lq=Lq, Lk=Lk, dk=dk, bias=self.bias, causal=causal, ldq=self.ldq, ldk=self.ldkv, ldv=self.ldkv)
        if drop is not None:  # (seed, tag, p): attention dropout on the probabilities
            self.seed = torch.tensor([drop[0]], dtype=torch.int32).cuda()
            self.kw.update(seed=self.seed, tag=drop[1], drop_p=drop[2])

    def forward(self, ops):
        ctx = MatOut(self.nb * self.Lq, H * self.dk, 1, self.dtype, H)
        lse = FlatOut(self.nb * H * self.Lq, torch.float32)
        ops.t5_attn_fwd(self.q, self.k, self.v, ctx.views[0], lse.view, ldo=ctx.ld, **self.kw)
        torch.cuda.synchronize()
        return ctx.fetch(self.Lq)[0], lse.fetch().reshape(self.nb, H, self.Lq)

    def backward(self, ops, ctx, lse, mode):
        """mode: 'none' (no bias gradient), 'atomics' (dbias, no scratch), 'ds_ws' (stored dS + reduce inside the call), 'ds_defer'
        (stored dS, klab_dbias_reduce called here).  ctx [B, H, Lq, dk] fp64 / lse fp64: what the forward left behind.
        -> dict of dq, dk, dv [B, H, L, dk], dbias [H, Lq, Lk], ds [B, H, Lq, Lk] (the stored slab, pad columns cut)"""
        Lq, Lk, dk = self.Lq, self.Lk, self.dk
        Lkp = (Lk + 31) // 32 * 32
        cbuf, ldc, (cv, dov) = fused_input([ctx, self.do], self.dtype)
        dq = MatOut(self.nb * Lq, H * dk, 1, self.dtype, H)
        dkv = MatOut(self.nb * Lk, H * dk, 2, self.dtype, H)
        dbias = FlatOut(H * Lq * Lk, torch.float32, fill=0.0) if mode != "none" else None
        ds = FlatOut(self.nb * H * Lq * Lkp, torch.bfloat16) if mode in ("ds_ws", "ds_defer") else None
        lse_d = lse.float().cuda()
        ops.t5_attn_bwd(self.q, self.k, self.v, cv, lse_d, dov, dq.views[0], dkv.views[0], dkv.views[1], ldo=ldc, lddo=ldc, lddq=dq.ld,
                        lddk=dkv.ld, lddv=dkv.ld, dbias=None if dbias is None else dbias.view, ds_ws=None if ds is None else ds.view,
                        ds_defer=mode == "ds_defer", **self.kw)
        if mode == "ds_defer":
            torch.cuda.synchronize()
            assert float(dbias.buf[GUARD:GUARD + dbias.n].abs().max()) == 0.0, "ds_defer must leave dbias to the caller"
            ops.dbias_reduce(ds.view, dbias.view, nbatch=self.nb, H=H, Lq=Lq, Lk=Lk)
        torch.cuda.synchronize()
        out = dict(dq=dq.fetch(Lq)[0])
        out["dk"], out["dv"] = dkv.fetch(Lk)
        if dbias is not None:
            out["dbias"] = dbias.fetch().reshape(H, Lq, Lk)
        if ds is not None:
            out["ds"] = ds.fetch().reshape(self.nb, H, Lq, Lkp)[..., :Lk]
        return out


def path_of(dtype, Lq, Lk, dk, causal):
    """the backward kernel klab_t5_attn_bwd sends the shape to (the forward: 'mfma' for bf16, dk in the MFMA set and Lk <= 256)"""
    if dtype == "bf16" and dk in (16, 32, 64, 128):
        if R.mfma_bwd_fits(Lq, Lk, dk):
            return "mfma"
        if not causal and dk in (32, 64):
            return "flash"
    return "generic"


def run_fixture(ops, dtype, kind, n, Lq, Lk, dk, causal, modes, drop=None):
    f = R.attn_fixture(kind, B, H, Lq, Lk, dk, causal, n, 0, drop)
    tag = f"{kind} n={n} (Lq, Lk, dk) = ({Lq}, {Lk}, {dk}) causal={causal} {dtype}" + (f" dropout (seed, tag, p) = {drop}" if drop else "")
    pr = Problem(f.q, f.k, f.v, f.do, f.bias, DT[dtype], Lq, Lk, dk, causal, drop)
    ctx, lse = pr.forward(ops)
    assert_out(ctx, f.ctx, f"forward ctx, {tag}")
    assert_f32_close(lse, f.lse, f"forward lse, {tag}")
    absds = f.dS.abs()
    mags = dict(dq=absds @ f.k.abs(), dk=absds.transpose(-1, -2) @ f.q.abs(), dv=f.Pm.transpose(-1, -2) @ f.do.abs())
    for mode in modes:
        got = pr.backward(ops, f.ctx, f.lse, mode)
        for name, ref in (("dq", f.dq), ("dk", f.dk_), ("dv", f.dv)):
            assert_out(got[name], ref, f"backward {name} ({mode}), {tag}", mags[name])
        if "ds" in got:
            assert_bf16_equal(got["ds"], f.dS, f"stored dS ({mode}), {tag}")
        if "dbias" in got:
            if "ds" in got:  # a sum of exact bf16 values in f32: exact
                bad = got["dbias"].double() != f.dbias
                assert not bool(bad.any()), f"backward dbias ({mode}), {tag}: first wrong (h, q, key) = {first_bad(bad) if bool(bad.any()) else None}"
            else:
                assert_f32_close(got["dbias"], f.dbias, f"backward dbias ({mode}), {tag}", absds.sum(0))


def case_id(c):
    return "-".join(str(v) for v in c)


# ------------------------------------------------------------------------------------------------ one-workgroup MFMA kernels
# forward: t5_attn_fwd_mfma<dk, MT>, MT = 4 / 8 / 16 for Lk = 58 / 69 / 153.  backward: t5_attn_bwd_mfma<dk> with the bias gradient
# through float atomics (B = 3), through the stored-dS slab reduced inside the call, and through ds_defer + klab_dbias_reduce;
# where its images do not fit LDS (exact_ref.mfma_bwd_fits: dk = 128 beyond Lq, Lk = 33, 69; causal 153 at dk = 64) the generic
# bf16 kernel t5_attn_bwd_kernel<bf16> runs instead, which only has the atomics form.
MFMA_CASES = [(kind, n, *c) for c in R.ATTN_MFMA for kind, n in R.fixtures_for(c[2])]


@pytest.mark.parametrize("kind,n,Lq,Lk,dk,causal", MFMA_CASES, ids=[case_id(c) for c in MFMA_CASES])
def test_mfma_one_workgroup_kernels(ops, kind, n, Lq, Lk, dk, causal):
    modes = ("atomics", "ds_ws", "ds_defer") if path_of("bf16", Lq, Lk, dk, causal) == "mfma" else ("atomics",)
    run_fixture(ops, "bf16", kind, n, Lq, Lk, dk, causal, modes)


# the dropout mask, stated on its own (exact_ref.attn_drop_mult: element (seed, tag, slab = b H + h, q Lk + key)): at p = 0.5 the
# multiplier is 0 or 2 and the dyadic fixtures stay dyadic (ctx = (P M) V, dV = (P M)^T dO, dS = P (dP M - delta)).  These are the
# kernels the fused attention kernels are compared with elsewhere.
DROP_CASES = [(kind, n, *c) for c in R.ATTN_DROP for kind, n in R.fixtures_for(c[2])]


@pytest.mark.parametrize("kind,n,Lq,Lk,dk,causal", DROP_CASES, ids=[case_id(c) for c in DROP_CASES])
def test_mfma_one_workgroup_kernels_dropout_mask(ops, kind, n, Lq, Lk, dk, causal):
    assert path_of("bf16", Lq, Lk, dk, causal) == "mfma"
    run_fixture(ops, "bf16", kind, n, Lq, Lk, dk, causal, ("atomics", "ds_ws", "ds_defer"), drop=R.FUSED_DROP)


# ------------------------------------------------------------------------------------------------ streaming kernels
# flash_fwd_kernel (Lk padded to 320 > 256), flash_bwd_dq_kernel + flash_bwd_dkv_kernel (the one-workgroup images of 224 queries
# and 320 keys exceed 160 KiB at both head dims).  Four query blocks and five key blocks of 64, the last of each ragged.  The bias
# gradient exists only through the dS slab here; 'none' runs the kernels without either.  onehot_nobias: the BIAS = 0 instantiations
# (the issue's n = Lk fixture needs a power-of-two Lk, which cannot have a ragged last block, and its dS is not a bf16 number; a
# one-hot row made by the scores themselves works at any Lk).
FLASH_CASES = [(kind, n, *c) for c in R.ATTN_FLASH for kind, n in R.fixtures_for(c[2]) + (("onehot_nobias", 1),)]


@pytest.mark.parametrize("kind,n,Lq,Lk,dk,causal", FLASH_CASES, ids=[case_id(c) for c in FLASH_CASES])
def test_streaming_kernels(ops, kind, n, Lq, Lk, dk, causal):
    assert path_of("bf16", Lq, Lk, dk, causal) == "flash"
    run_fixture(ops, "bf16", kind, n, Lq, Lk, dk, causal, ("none",) if kind == "onehot_nobias" else ("none", "ds_ws", "ds_defer"))


# ------------------------------------------------------------------------------------------------ generic kernels (attn_t5.hip)
# t5_attn_fwd_kernel<T> / t5_attn_bwd_kernel<T>: f32 at Lq = 21, 37 (no multiple of TQ = 16), bf16 at head dim 24, and the f32
# backward in key chunks (kc = 112 < Lk = 153 at dk = 64)
GENERIC_CASES = [(c[0], kind, n, *c[1:]) for c in R.ATTN_GENERIC for kind, n in R.fixtures_for(c[3])]


@pytest.mark.parametrize("dtype,kind,n,Lq,Lk,dk,causal", GENERIC_CASES, ids=[case_id(c) for c in GENERIC_CASES])
def test_generic_kernels(ops, dtype, kind, n, Lq, Lk, dk, causal):
    assert path_of(dtype, Lq, Lk, dk, causal) == "generic"
    run_fixture(ops, dtype, kind, n, Lq, Lk, dk, causal, ("atomics", "none"))


# ------------------------------------------------------------------------------------------------ random operands, per element
RANDOM = [
    # (dtype, Lq, Lk, dk, causal, with_bias, modes)
    ("bf16", 70, 153, 64, False, True, ("ds_ws", "atomics")),   # t5_attn_fwd_mfma<64, 16>, t5_attn_bwd_mfma<64>
    ("bf16", 69, 69, 64, True, True, ("ds_ws",)),               # the same kernels with the causal mask, MT = 8
    ("bf16", 33, 69, 128, False, True, ("ds_defer",)),          # dk = 128
    ("bf16", 200, 300, 64, False, True, ("ds_ws",)),            # flash_fwd / flash_bwd_dq / flash_bwd_dkv <64, 1>
    ("bf16", 200, 300, 32, False, False, ("none",)),            # <32, 0>
    ("bf16", 33, 58, 24, False, True, ("atomics",)),            # generic bf16 kernels
    ("f32", 37, 37, 32, True, True, ("atomics",)),              # generic f32 kernels
    ("f32", 33, 153, 64, False, True, ("atomics",)),            # ... the chunked backward
]


@pytest.mark.parametrize("dtype,Lq,Lk,dk,causal,with_bias,modes", RANDOM, ids=[case_id(c[:6]) for c in RANDOM])
def test_random_operands_per_element(ops, dtype, Lq, Lk, dk, causal, with_bias, modes):
    d = R.attn_randn(B, H, Lq, Lk, dk, causal, with_bias)
    q, k, v, do = d["q"], d["k"], d["v"], d["do"]
    pr = Problem(q, k, v, do, d["bias"], DT[dtype], Lq, Lk, dk, causal)
    path = path_of(dtype, Lq, Lk, dk, causal)
    print(f"\nattention randn {dtype} (Lq, Lk, dk) = ({Lq}, {Lk}, {dk}) causal={causal} bias={with_bias}: backward path {path}")
    ctx, lse = pr.forward(ops)
    f32f = R.attn_f32_factor(q, k, Lk, dk)
    f32b = R.attn_f32_bounds(dict(P=d["P"], D=d["P"]), q, k, v, do, Lq, Lk, dk, B)["ctx"]
    # bf16 MFMA / streaming kernels: P and the output are rounded; the generic bf16 kernel keeps P in f32 and rounds the output only
    if dtype == "f32":
        cb = f32b
    elif path == "generic":
        cb = R.U8 * d["ctx"].abs() + f32b
    else:
        cb = R.attn_fwd_bound(d["P"], v)
    worst = [ratio(ctx, d["ctx"], cb, "ctx")]
    vis = f32f if not causal else f32f.masked_fill((torch.arange(Lk)[None, :] > torch.arange(Lq)[:, None])[None, None], 0.0)
    worst.append(ratio(lse, d["lse"], vis.amax(-1) + 4.0 * R.U24 * d["lse"].abs(), "lse"))
    # the backward is a function of what the forward left behind: feed the reference the kernel's own ctx and lse
    ctx64, lse64 = ctx.double(), lse.double()
    r = R.attn_backward_reference(q, k, v, d["bias"], causal, ctx64, lse64, do)
    for mode in modes:
        got = pr.backward(ops, ctx64, lse64, mode)
        if dtype == "f32":
            bnd = R.attn_f32_bounds(r, q, k, v, do, Lq, Lk, dk, B)
        elif path == "generic":  # f32 arithmetic on bf16 inputs, one rounding at the store; dbias is f32 atomics
            fb = R.attn_f32_bounds(r, q, k, v, do, Lq, Lk, dk, B)
            bnd = {n_: R.U8 * r[n_].abs() + fb[n_] for n_ in ("dq", "dk", "dv")}
            bnd["dbias"] = fb["dbias"]
        else:
            bnd = R.attn_bwd_bounds(r, q, k, v, do, Lq, Lk, dk, B, stored_ds="ds" in got)
        for name in ("dq", "dk", "dv") + (("dbias",) if "dbias" in got else ()):
            worst.append(ratio(got[name], r[name], bnd[name], f"{name} ({mode})"))
    bad = [msg for v_, msg in worst if not v_ <= 1.0]
    assert not bad, bad
