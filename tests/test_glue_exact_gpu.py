"""Exact tests of the streaming kernels of csrc/misc.hip: every one of them is a move (torch.equal with the gathered source) or a sum
of small integers (exact in f32 in any order, torch.equal with the fp64 sum).  Every output lies between guard bands
(rowops_ref.Guarded); the dropout sites are compared with rowops_ref.drop_mult at index row * d + c.

rule                                                        -> shape
  embed: one wave per row, 4 columns per lane, 256 a sweep  -> d = 4, 260; rows = 18 (three sequences of L = 6), 8200 (second lap at 8192)
  stream_grid: 2048 workgroups of 256, then grid-stride     -> 2048 * 256 work items + a tail (convert, add_f32, merge_gather / scatter)
  im2col: P = 4 has its own kernel behind the _ld entry     -> P = 4 at ldo = 48 and 64 (zero tail), P = 2, 8 through the generic one
  colsum: f32 / unaligned bf16 scalar, aligned bf16 8-wide  -> N = 100, a column offset of 4 elements, column slices; M = 1, 300, 70000"""
import pytest
import torch

from tests import rowops_ref as R
from tests.rowops_ref import U24, Guarded, assert_equal, assert_within

pytestmark = pytest.mark.gpu

SEED, BF16, F32 = 4321, torch.bfloat16, torch.float32
LAP = 2048 * 256  # work items of one lap of a streaming kernel


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


@pytest.fixture(scope="module")
def seed():
    return torch.tensor([SEED], dtype=torch.int32).cuda()


# ---------------------------------------------------------------------------------------------------------------- embedding
VOCAB, L_SEQ, START, PAD = 50, 6, 7, 3


def _ids(rows, g):
    ids = torch.randint(0, VOCAB, (rows,), generator=g)
    ids[::5] = ids[0]  # repeated ids
    return ids


def _effective_ids(ids, shift):
    if not shift:
        return ids.clone()
    eff = torch.roll(ids, 1)
    eff[torch.arange(len(ids)) % L_SEQ == 0] = START
    eff[eff == -100] = PAD
    return eff


@pytest.mark.parametrize("rows", [18, 8200])
@pytest.mark.parametrize("d", [4, 260])
@pytest.mark.parametrize("shift", [False, True], ids=["plain", "shift_right"])
def test_embed_fwd_and_bwd(ops, seed, rows, d, shift):
    g = R.gen(8000 + rows + d)
    table = torch.randn(VOCAB, d, generator=g)
    ids = _ids(rows, g)
    if shift:
        ids[4] = -100   # a label position: read as the pad id by the row after it
        ids[5] = -100   # the last of its sequence: read by nobody (row 6 takes the start id)
    eff = _effective_ids(ids, shift)
    tag = f" rows={rows} d={d} shift={shift}"
    kw = dict(shift_right=shift, L_seq=L_SEQ, start_id=START, pad_id=PAD)
    ids_d, table_d = ids.cuda(), table.cuda()
    for p in (0.0, 0.5):
        m = R.mask(SEED, 21, p, R.remap_rows(rows), d) if p else None
        out, err = Guarded((rows, d), F32), Guarded((1,), torch.int32, init=torch.zeros(1, dtype=torch.int32))
        ops.embed_fwd(ids_d, table_d, out.t, drop_p=p, seed=seed, tag=21, err=err.t, **kw)
        want = table[eff] if m is None else table[eff] * m
        got = out.check("out")
        if p:
            assert_equal("embed_fwd mask", got != 0, m != 0, tag)
        assert_equal(f"embed_fwd out p={p}", got, want, tag)
        assert int(err.check("err")) == 0, f"embed_fwd{tag}: err flag set on valid ids"
        # backward: integer dh onto a nonzero integer table
        dh = R.ints(g, -3, 3, rows, d)
        dt0 = R.ints(g, 1, 5, VOCAB, d)
        dt = Guarded((VOCAB, d), F32, init=dt0.float())
        ops.embed_bwd(ids_d, dh.float().cuda(), dt.t, drop_p=p, seed=seed, tag=21, **kw)
        wantb = dt0.clone().index_add_(0, eff, dh if m is None else dh * m.double())
        assert_equal(f"embed_bwd dtable p={p}", dt.check("dtable").double(), wantb, tag)


def test_embed_out_of_range_id(ops):
    g = R.gen(8100)
    rows, d = 18, 260
    table = torch.randn(VOCAB, d, generator=g)
    ids = _ids(rows, g)
    ids[7], ids[11] = VOCAB, -1
    eff = ids.clone()
    eff[7] = eff[11] = 0
    out, err = Guarded((rows, d), F32), Guarded((1,), torch.int32, init=torch.zeros(1, dtype=torch.int32))
    ops.embed_fwd(ids.cuda(), table.cuda(), out.t, err=err.t)
    assert_equal("embed_fwd out (id out of range reads row 0)", out.check("out"), table[eff])
    assert int(err.check("err")) == 1
    dh, dt0 = R.ints(g, -3, 3, rows, d), R.ints(g, 1, 5, VOCAB, d)
    dt = Guarded((VOCAB, d), F32, init=dt0.float())
    ops.embed_bwd(ids.cuda(), dh.float().cuda(), dt.t)
    ok = (ids >= 0) & (ids < VOCAB)
    assert_equal("embed_bwd dtable (id out of range skipped)", dt.check("dtable").double(), dt0.clone().index_add_(0, ids[ok], dh[ok]))


# ---------------------------------------------------------------------------------------------------------------- position bias
@pytest.mark.parametrize("Lq,Lk", [(9, 13), (70, 70)])
@pytest.mark.parametrize("nb", [32, 64])
def test_relbias_fwd_and_bwd(ops, Lq, Lk, nb):
    H = 3
    g = R.gen(8200 + Lq + nb)
    table = torch.randn(nb, H, generator=g)
    bucket = torch.randint(0, nb, (Lq, Lk), generator=g, dtype=torch.int32)
    bucket[0, 0], bucket[-1, -1] = nb - 1, 0
    bias = Guarded((H, Lq, Lk), F32)
    ops.relbias_fwd(table.cuda(), bucket.cuda(), bias.t)
    assert_equal("relbias_fwd bias", bias.check("bias"), table[bucket.long()].permute(2, 0, 1).contiguous(), f" {Lq}x{Lk} nb={nb}")
    dbias, dt0 = R.ints(g, -3, 3, H, Lq, Lk), R.ints(g, 1, 5, nb, H)
    dt = Guarded((nb, H), F32, init=dt0.float())
    ops.relbias_bwd(dbias.float().cuda(), bucket.cuda(), dt.t)
    want = dt0.clone()
    want.index_add_(0, bucket.long().flatten(), dbias.reshape(H, -1).T.contiguous())
    assert_equal("relbias_bwd dtable", dt.check("dtable").double(), want, f" {Lq}x{Lk} nb={nb}")


def test_relbias_bwd_refuses_more_than_64_buckets(ops):
    with pytest.raises(Exception):
        ops.relbias_bwd(torch.zeros(3, 4, 4).cuda(), torch.zeros(4, 4, dtype=torch.int32).cuda(), torch.zeros(65, 3).cuda())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- im2col
def _im2col_ref(pix, P):
    B, Cin, Hh, _ = pix.shape
    Rr = Hh // P
    # [B, Cin, y, py, x, px] -> [B, y, x, Cin, py, px]
    return pix.view(B, Cin, Rr, P, Rr, P).permute(0, 2, 4, 1, 3, 5).reshape(B * Rr * Rr, Cin * P * P).contiguous()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("P,ldo,direct", [(4, 48, True), (4, 64, False), (4, 48, False), (2, 12, False), (8, 192, False)],
                         ids=["p4_ld48_own_kernel", "p4_ld64_own_kernel", "p4_generic", "p2_generic", "p8_generic"])
def test_im2col_patch(ops, dtype, P, ldo, direct):
    from klab_multimodalmodel_amd import _lib as L
    B, Cin, Hh = 2, 3, 5 * P
    g = R.gen(8300 + P)
    pix = torch.randn(B, Cin, Hh, Hh, generator=g)
    K = Cin * P * P
    out = Guarded((B * 25, ldo), dtype)
    pix_d = pix.cuda()
    if direct:  # ops.im2col_patch sends ldo == K to the generic kernel; the P = 4 kernel is reached through the _ld entry
        L.check(L.load().klab_im2col_patch_ld(pix_d.data_ptr(), out.t.data_ptr(), L.dtype_code(dtype), B, Cin, Hh, P, ldo, L.stream_ptr()),
                "klab_im2col_patch_ld")
    else:
        ops.im2col_patch(pix_d, out.t, P)
    want = torch.zeros(B * 25, ldo)
    want[:, :K] = _im2col_ref(pix, P)
    assert_equal("im2col_patch out", out.check("out"), want.to(dtype), f" P={P} ldo={ldo} {dtype}")


# ---------------------------------------------------------------------------------------------------------------- patch merging
def _merge_ref(x):
    return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).flatten(1, 2).contiguous()


@pytest.mark.parametrize("B,Rr,C", [(2, 2, 4), (2, 14, 4), (3, 2, 96), (2, 14, 96), (8, 56, 96)])
def test_merge_gather_and_scatter(ops, B, Rr, C):
    assert (B, Rr, C) != (8, 56, 96) or B * (Rr // 2) ** 2 * C > LAP  # the second lap
    g = R.gen(8400 + Rr + C)
    x = torch.randn(B, Rr, Rr, C, generator=g)
    want = _merge_ref(x)
    tag = f" B={B} R={Rr} C={C}"
    for dtype in (BF16, F32):
        out = Guarded(tuple(want.shape), dtype)
        ops.merge_gather(x.cuda(), out.t, B=B, R=Rr, C=C)
        assert_equal(f"merge_gather out ({dtype})", out.check("out"), want.to(dtype), tag)
    dx = Guarded((B, Rr, Rr, C), F32)
    ops.merge_scatter(want.cuda(), dx.t, B=B, R=Rr, C=C)
    assert_equal("merge_scatter dx", dx.check("dx"), x, tag)


def test_merge_refuses_odd_resolution(ops):
    x = torch.zeros(1, 3, 3, 4).cuda()
    with pytest.raises(Exception):
        ops.merge_gather(x, torch.zeros(1, 1, 16).cuda(), B=1, R=3, C=4)
    with pytest.raises(Exception):
        ops.merge_scatter(torch.zeros(1, 1, 16).cuda(), x, B=1, R=3, C=4)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- convert, add
@pytest.mark.parametrize("n", [4, 1028, LAP * 4 + 8])
def test_convert_and_add_f32(ops, n):
    g = R.gen(8500)
    x = torch.randn(n, generator=g)
    x_d = x.cuda()
    for scale in (1.0, 0.5, 0.3):
        s = torch.tensor(scale, dtype=F32)
        for dtype in (BF16, F32):
            y = Guarded((n,), dtype)
            ops.convert(x_d, y.t, scale)
            assert_equal(f"convert y ({dtype}, scale {scale})", y.check("y"), (x * s).to(dtype), f" n={n}")
    y0 = torch.randn(n, generator=g)
    y = Guarded((n,), F32, init=y0)
    ops.add_f32(y.t, x_d)
    assert_equal("add_f32 y", y.check("y"), y0 + x, f" n={n}")


def test_add_f32_refuses_a_ragged_length(ops):
    with pytest.raises(Exception):
        ops.add_f32(torch.zeros(6).cuda(), torch.zeros(6).cuda())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- column sums
# (dtype, N, columns of the matrix it is a slice of, first column of the slice)
COLSUM = [(F32, 100, 100, 0), (F32, 132, 200, 20), (BF16, 136, 136, 0), (BF16, 64, 200, 8), (BF16, 100, 100, 0), (BF16, 128, 136, 4)]


@pytest.mark.parametrize("M", [1, 300, 70000])
@pytest.mark.parametrize("dtype,N,ld,c0", COLSUM, ids=["f32", "f32_slice", "bf16_8wide", "bf16_8wide_slice", "bf16_N100_scalar", "bf16_offset4_scalar"])
def test_colsum_exact_on_integers(ops, M, dtype, N, ld, c0):
    g = R.gen(8600 + M + N)
    full = R.ints(g, -3, 3, M, ld)
    out0 = R.ints(g, 1, 5, N)
    full_d = full.to(dtype).cuda()
    out = Guarded((N,), F32, init=out0.float())
    ops.colsum(full_d[:, c0:c0 + N], out.t)
    assert_equal("colsum out", out.check("out").double(), out0 + full[:, c0:c0 + N].sum(0), f" M={M} N={N} ld={ld} c0={c0} {dtype}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_colsum_randn_per_element(ops, dtype):
    M, N = 3000, 136
    g = R.gen(8700)
    x = torch.randn(M, N, generator=g).to(dtype)
    out = Guarded((N,), F32, init=torch.zeros(N))
    ops.colsum(x.cuda(), out.t)
    assert_within(f"colsum out (randn, {dtype})", out.check("out"), x.double().sum(0), 2 * M * U24 * x.double().abs().sum(0))


# ---------------------------------------------------------------------------------------------------------------- GEMM epilogue mask
@pytest.mark.parametrize("dtype,K,name_tag", [(F32, 72, 0), (BF16, 96, 0), (BF16, 192, 2)], ids=["f32", "bf16_ring", "bf16_256x256"])
def test_gemm_epilogue_dropout_mask_is_the_hash_at_m_N_plus_n(ops, seed, dtype, K, name_tag):
    from tests import exact_ref as E
    M, N = E.EPI
    A, B, prod = E.gemm_ints(M, N, K)
    out = Guarded((M, N), F32)
    ops.gemm(A.to(dtype).cuda(), B.to(dtype).cuda(), out.t, M=M, N=N, K=K, drop_p=0.5, seed=seed, tag=31, name_tag=name_tag)
    m = R.mask(SEED, 31, 0.5, R.remap_rows(M), N)
    assert_equal("gemm C (dropout p = 0.5)", out.check("C").double(), prod * m.double(), f" K={K} {dtype} name_tag={name_tag}")
    assert int((prod != 0).sum()) > M * N // 2  # (enough non-zero products for the mask to be visible)
