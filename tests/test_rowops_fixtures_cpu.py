"""What the GPU tests of the row kernels take for granted about tests/rowops_ref.py, proved without a GPU: the dropout hash has the
rate and the sensitivity it should, the backward fixtures are exact in f32 whatever the evaluation order, and the bounds are
positive where they are used."""
import numpy as np
import pytest
import torch

from tests import rowops_ref as R


# ---- the dropout hash ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,tag", [(1234, 0), (1234, 7), (99, 7)])
@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_drop_mult_keep_rate_and_scale(seed, tag, p):
    m = R.drop_mult(seed, tag, p, np.arange(1 << 17))
    assert m.dtype == np.float32
    keep = float((m != 0).mean())
    assert abs(keep - (1.0 - p)) < 0.01, keep
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert set(np.unique(m).tolist()) == {0.0, float(scale)}
    if p == 0.5:
        assert float(scale) == 2.0


def test_drop_mult_depends_on_seed_tag_and_the_high_word():
    idx = np.arange(1 << 14)
    base = R.drop_mult(1234, 3, 0.5, idx)
    for other in (R.drop_mult(1235, 3, 0.5, idx), R.drop_mult(1234, 4, 0.5, idx), R.drop_mult(1234, 3, 0.5, idx + (1 << 32))):
        differ = float((other != base).mean())
        assert 0.4 < differ < 0.6, differ  # independent masks at p = 0.5 differ on half the elements
    # the high-word round is applied only where the high word is not zero
    assert np.array_equal(R.drop_hash(1234, 3, idx), R.mix32((idx.astype(np.uint64) * np.uint64(0x9E3779B1) + R.mix32(
        np.uint64((1234 * 0x9E3779B1 + 3 * 0x7FEB352D + 0x165667B1) & 0xFFFFFFFF))) & R.M32))


def test_mix32_known_values_and_threshold():
    # murmur3's finaliser: 0 is its fixed point, and it is a bijection (no collisions on a sample)
    assert int(R.mix32(np.uint64(0))) == 0
    v = R.mix32(np.arange(1 << 16))
    assert len(np.unique(v)) == 1 << 16 and int(v.max()) < 1 << 32
    assert (R.drop_mult(1, 1, 1e-12, np.arange(4096)) != 0).all()        # threshold 0: nothing dropped
    assert float((R.drop_mult(1, 1, 0.999, np.arange(1 << 15)) != 0).mean()) < 0.01


def test_remap_and_mask_index():
    assert R.remap_rows(7, **R.REMAP).tolist() == [1, 2, 3, 6, 7, 8, 11]
    assert R.out_rows(7, **R.REMAP) == 12 and R.out_rows(7) == 7
    m = R.mask(5, 6, 0.5, R.remap_rows(4, **R.REMAP), 12)
    want = R.drop_mult(5, 6, 0.5, np.array([[r * 12 + c for c in range(12)] for r in (1, 2, 3, 6)]))
    assert np.array_equal(m.numpy(), want)


def test_adds():
    assert R.adds(132) == 4 * 1 + 6 + 4 and R.adds(260) == 4 * 2 + 6 + 4 and R.adds(64, 16) == 4 + 4 + 4
    assert [R.ln_lanes(C) for C in (4, 64, 68, 128, 132)] == [16, 16, 32, 32, 64]


# ---- the backward fixtures are exact -------------------------------------------------------------------------------------------
def f32_exact(x):
    return bool((x.float().double() == x).all())


@pytest.mark.parametrize("rows,d", sorted(set(R.RMS_BWD + [(r, d) for r, d, _ in R.RMS_BWD_SPLIT])))
def test_rms_bwd_fixture_is_exact(rows, d):
    fx = R.rms_bwd_fixture(rows, d)
    my = torch.from_numpy(R.drop_mult(1, 2, 0.5, np.arange(rows * d).reshape(rows, d)))
    mp = torch.from_numpy(R.drop_mult(1, 3, 0.5, np.arange(rows * d).reshape(rows, d)))
    for m in (None, my):
        e = R.rms_bwd_exact(fx, m, mp)
        # the dot product and all its partial sums are integers below 2^24: exact in any order
        terms = e["de"] * fx["w"][None] * fx["x"]
        assert bool((terms == terms.round()).all()) and float(terms.abs().sum(-1).max()) < 2 ** 24
        assert f32_exact(e["dot"] * fx["rstd"] ** 3)                          # one rounding in k: the division
        assert f32_exact(fx["rstd"][:, None] * fx["w"][None] * e["de"])       # r w de exact
        assert f32_exact(fx["x"] * e["k"].double()[:, None])                  # x k exact
        assert torch.equal(R.rms_bwd_fma(fx, m, mp), e["dx"])                 # fused multiply-add order gives the same bits
        # weight gradient: multiples of 1/4, absolute column sums below 2^17 quarters x 8 (2^24 at the very most), onto dw0
        wt = (e["de"] * fx["x"] * fx["rstd"][:, None]) * 4
        assert bool((wt == wt.round()).all()) and float(wt.abs().sum(0).max()) + 4 * 5 < 2 ** 24
        assert float(wt.abs().sum(0).max()) < 2 ** 17 * 8
        assert f32_exact(fx["dw0"] + e["dwsum"])
        assert f32_exact(e["dxt32"].double())
    assert bool((fx["dw0"] != 0).all())


# (rows, C, seed of the fixture): the fused, the split-subset and the wide-row tests
LN_BWD_ALL = [(r, C, 0) for r, C in R.LN_BWD + [R.LN_DPREV_EXACT]] + [(r, C, 1) for r, C in R.LN_BWD_SUBSETS] + [(r, C, 2) for r, C, _ in R.LN_BWD_SPLIT]


@pytest.mark.parametrize("rows,C,seed", LN_BWD_ALL)
def test_ln_bwd_fixture_is_exact(rows, C, seed):
    fx = R.ln_bwd_fixture(rows, C, seed)
    m = torch.from_numpy(R.drop_mult(1, 2, 0.5, np.arange(rows * C).reshape(rows, C)))
    for mm in (None, m):
        e = R.ln_bwd_exact(fx, mm)
        assert f32_exact(fx["y"]) and bool((fx["y"].to(torch.bfloat16).double() == fx["y"]).all())  # both input dtypes hold y
        gd = fx["gamma"][None] * e["de"]
        assert float(gd.abs().sum(-1).max()) < 2 ** 24 and float((gd * e["xh"]).abs().sum(-1).max()) * 4 < 2 ** 24
        assert f32_exact(e["s1n"]) and f32_exact(e["s2n"])
        assert f32_exact(e["xh"] * e["s2"].double()[:, None])             # xhat s2 exact
        assert torch.equal(R.ln_bwd_fma(fx, mm), e["dy"])
        wt = e["de"] * e["xh"] * 4
        assert bool((wt == wt.round()).all()) and float(wt.abs().sum(0).max()) + 20 < 2 ** 24
        assert f32_exact(fx["dgamma0"] + e["dgamma"]) and f32_exact(fx["dbeta0"] + e["dbeta"])


def test_forward_fixtures():
    fx = R.ln_randn(5, 132)
    assert bool((fx["y"].to(torch.bfloat16).float() == fx["y"]).all())
    assert set(fx["gamma"].tolist()) <= set(R.GAMMAS)
    assert bool((fx["yi"] == fx["yi"].round()).all())
    # a column lost from a 132-wide row moves rstd by far more than the bound allows
    x = R.rms_randn(5, 132)["x"].double()
    r = (x.pow(2).mean(-1) + 1e-6).rsqrt()
    r_lost = ((x[:, :-1].pow(2).sum(-1)) / 132 + 1e-6).rsqrt()
    assert float(((r_lost - r).abs() / ((R.adds(132) + 8) * R.U24 * r)).median()) > 100
    ref, bound = R.ln_fwd_reference(fx["y"], fx["gamma2"], fx["beta"], fx["shortcut"], 132)
    assert bool((bound > 0).all()) and float((bound / (ref.abs() + 1)).max()) < 1e-3


def test_q8_expected():
    y = torch.tensor([[0.0, 0.0, 0.0, 0.0], [1.0, -2.0, 448.0, 0.5], [-3.0, 1.5, 0.25, 0.0]]).to(torch.bfloat16)
    b, sc = R.q8_expected(y)
    assert sc.tolist() == [1.0, 1.0, float(torch.tensor(3.0) * torch.tensor(1.0 / 448.0))]
    assert b[0].tolist() == [0, 0, 0, 0]
    assert b[1].view(torch.float8_e4m3fn).float().tolist() == [1.0, -2.0, 448.0, 0.5]
    assert float(b[2].view(torch.float8_e4m3fn).float()[0]) == -448.0
    assert R.unsigned_zero(torch.tensor([0x80, 0x81, 0], dtype=torch.uint8)).tolist() == [0, 0x81, 0]


def test_ln_bwd_dprev_is_exact_at_a_power_of_two_width():
    # C = 64: s1 and s2 are divided by a power of two, so dy is dyadic; with every partial column sum (onto dprev0) below 2^24
    # granules the sum is exact in any order
    rows, C = R.LN_DPREV_EXACT
    fx = R.ln_bwd_fixture(rows, C)
    dy = R.ln_bwd_exact(fx)["dy"].double()
    k = next(k for k in range(40) if bool((dy * 2.0 ** k == (dy * 2.0 ** k).round()).all()))
    assert (float(dy.abs().sum(0).max()) + 5) * 2.0 ** k < 2 ** 24, k
