"""What tests/test_frozen_tower_exact_gpu.py takes for granted about tests/frozen_tower_ref.py, proved without a GPU:
  - gelu_poly (common.h, restated in numpy f32) is max(u, 0) bit for bit on the lattice the fixtures use, with and without fused
    multiply-adds, and errs by at most 1.2e-4 anywhere (the Level 2 term);
  - every integer fixture is exact: operands held by bf16, product sums below 2^24, hidden rows held by bf16, the pre-norm row held
    by bf16 where the kernel rounds it, the row mean exactly mu, d = 1 with gamma = 1, beta = 0, shortcut = 0 at the probe, and the
    output expression the same in both multiply-add orders;
  - the coverage conditions: every hidden unit positive, negative and zero somewhere; every input column non-zero in a row that
    reaches a non-zero last-layer weight; every element of every operand, moved by one lattice step, changes an expected output
    (analytically for every master fixture, and by recomputing the fp64 reference on a sample for every kernel and width);
  - the Level 2 bound holds against the worst-case sign pattern of +-delta_y and is not slack by more than a factor of two, and a
    parameter vector shifted by one index leaves it."""
import numpy as np
import pytest
import torch

from tests import frozen_tower_ref as T
from tests.exact_ref import bf16_exact, gen
from tests.rowops_ref import GAMMAS, gelu_erf64

MASTERS = ([("proj", C, mu) for C in (64, 128) for mu in T.MUS] + [("mlp", C, mu) for C in (64, 128) for mu in T.MUS]
           + [("linear_ln", K, mu) for K in T.LINLN_M for mu in T.MUS]
           + [("patch_embed", (B, HW, C), mu) for B, HW in T.EMBED_SHAPES for C in (64, 96, 128) for mu in T.MUS if C != 96 or mu == 0])


def master(kernel, key, mu):
    if kernel == "proj":
        return T.proj_fixture(key, mu)
    if kernel == "mlp":
        return T.mlp_fixture(key, mu)
    if kernel == "linear_ln":
        return T.linln_fixture(key, mu)
    return T.embed_fixture(*key, mu)


def f32_exact(x):
    return bool((x.float().double() == x).all())


# ---- GELU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fma", [False, True])
def test_gelu_poly_is_relu_on_the_lattice(fma):
    top = max(float(T.mlp_fixture(C, mu)["u"].abs().max()) for C in (64, 128) for mu in T.MUS)
    assert top <= 4096
    u = np.arange(-4096, 4097).astype(np.float32)
    u = u[(np.abs(u) >= 5) | (u == 0)]  # every integer of the range, not only the multiples of 8 in use
    got = T.gelu_poly_np(u, fma)
    assert got.dtype == np.float32 and np.array_equal(got, np.maximum(u, 0))
    assert not np.signbit(got).any()  # negative u gives +0
    for C in (64, 128):
        for mu in T.MUS:
            fx = T.mlp_fixture(C, mu)
            uu = fx["u"].numpy()
            assert bool((uu % 8 == 0).all())
            assert np.array_equal(T.gelu_poly_np(uu.astype(np.float32), fma).astype(np.float64), fx["h"].numpy())


@pytest.mark.parametrize("fma", [False, True])
def test_gelu_poly_error_is_below_the_level_2_term(fma):
    u = np.linspace(-45.0, 45.0, 900001).astype(np.float32)
    err = np.abs(T.gelu_poly_np(u, fma).astype(np.float64) - gelu_erf64(torch.from_numpy(u)).numpy())
    assert float(err.max()) <= T.GELU_POLY_ERR, (float(err.max()), float(u[err.argmax()]))
    x = torch.linspace(-8, 8, 160001, dtype=torch.float64, requires_grad=True)
    (slope,) = torch.autograd.grad(gelu_erf64(x).sum(), x)
    assert 1.12 < float(slope.abs().max()) <= T.GELU_SLOPE


# ---- exactness -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,key,mu", MASTERS)
def test_fixture_is_exact(kernel, key, mu):
    fx = master(kernel, key, mu)
    C, M = fx["C"], fx["x"].shape[0]
    for k in ("x", "W") + (("W1",) if kernel == "mlp" else ()):
        assert bf16_exact(fx[k]), k
    for k in ("b", "gamma", "beta", "sc") + (("b1",) if kernel == "mlp" else ()):
        assert f32_exact(fx[k]) and bool((fx[k] * 2 == (fx[k] * 2).round()).all()), k
    assert float(fx["absacc"].max()) < 2 ** 24  # every partial sum in any order is an integer f32 holds
    if kernel == "mlp":
        assert float(fx["absu"].max()) < 2 ** 24 and bool((fx["u"] % 8 == 0).all())
        assert torch.equal(fx["h"], fx["u"].clamp_min(0.0)) and bf16_exact(fx["h"])  # the RNE of the hidden store changes nothing
    if kernel == "patch_embed":
        assert bool((fx["pix"].float().bfloat16().double() == fx["pix"]).all())
        B, HW = key[0], key[1]
        R = HW // 4
        m = M - 1  # the layout: patch row m, element k = 16 c + 4 dy + dx
        b, py, px = m // (R * R), (m % (R * R)) // R, m % R
        for k in (0, 5, 17, 47):
            assert float(fx["pix"][b, k // 16, py * 4 + (k % 16) // 4, px * 4 + k % 4]) == float(fx["x"][m, k])
    if kernel in ("linear_ln", "patch_embed"):  # y = bf16(acc + bias): exact while |y| <= 256
        assert float(fx["y"].abs().max()) <= 256 and bf16_exact(fx["y"])
    # the mean is mu exactly: the row sum is C mu, an integer, and sum * f32(1 / C) is exact for a power of two C (or a zero sum)
    assert bool((fx["y"].sum(-1) == C * mu).all())
    assert C & (C - 1) == 0 or mu == 0
    rowsum = fx["y"].sum(-1).float()
    assert torch.equal(rowsum * torch.tensor(1.0 / C, dtype=torch.float32), torch.full((M,), float(mu)))
    assert bool((fx["d"] == fx["d"].round()).all()) and float(fx["d"].abs().max()) < 2 ** 12  # d^2 sums stay far below 2^53
    # the probe
    rows = torch.arange(M)
    p = fx["probe"]
    assert bool((fx["d"][rows, p] == 1).all()) and bool((fx["gamma"][p] == 1).all()) and bool((fx["beta"][p] == 0).all())
    assert bool((fx["sc"][rows, p] == 0).all())
    if M >= 2 * T.NPROBE:
        assert len(set(p.tolist())) == T.NPROBE
        for q in T.probe_channels(C):  # in the rows where q is not the probe it is a channel like any other
            other = p != q
            assert bool((fx["d"][other, q] != 1).any())
            assert kernel == "patch_embed" or bool((fx["sc"][other, q] != 0).all())
    assert set(fx["gamma"].tolist()) <= set(GAMMAS)
    assert bool(((fx["var"] * C) == (fx["var"] * C).round()).all()) or C == 96
    # both multiply-add orders, at the fp64 rstd and at values a few ulp to either side
    rho = fx["rho"].float()
    for k in (-3, 0, 2):
        r = rho
        for _ in range(abs(k)):
            r = torch.nextafter(r, torch.full_like(r, float("inf") if k > 0 else 0.0))
        a, b = T.expected_out(fx, r), T.expected_out(fx, r, fma=True)
        assert torch.equal(a, b)
        assert torch.equal(a[rows, p], r)  # the probe reads rho back unrounded


def test_prefixes_share_the_master():
    fx = T.mlp_fixture(64, 3)
    sub = T.take_rows(fx, 33)
    assert sub["x"].shape[0] == 33 and sub["W1"] is fx["W1"] and torch.equal(sub["rho"], fx["rho"][:33])
    assert T.chain("mlp", 64) == 18 and T.chain("proj", 128) == 34 and T.chain("patch_embed", 96) == 26 and T.chain("linear_ln", 256) == 69


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def big(kernel, key):
    """masters with enough rows to carry the coverage proof (their weights are what every smaller case runs)"""
    return kernel != "patch_embed" or key[:2] == (5, 28)


@pytest.mark.parametrize("kernel,key,mu", [m for m in MASTERS if big(m[0], m[1])])
def test_coverage_conditions(kernel, key, mu):
    fx = master(kernel, key, mu)
    x, W, d, gamma = fx["x"], fx["W"], fx["d"], fx["gamma"]
    live_gamma = (gamma != 0)
    assert int(live_gamma.sum()) > gamma.numel() // 2
    # a change of y[r, c] always shows: d[r, c] moves by (1 - 1 / C) of it and gamma[c] != 0, or else every other d of the row
    # moves by 1 / C of it and rho moves, and some of those channels have gamma != 0 and d != 0
    assert bool(((d != 0) & live_gamma[None]).any(-1).all())
    a = fx["h"] if kernel == "mlp" else x
    # W[c, k] + 1 moves y[:, c] by a[:, k]: every input column of the last Linear is non-zero in some row ...
    assert bool((a != 0).any(0).all())
    # ... and reaches a non-zero weight (so a wrong input element shows as well)
    assert bool((W != 0).any(0).all())
    # gamma[c] one lattice step on: out[:, c] moves by d rho times the step wherever d != 0; beta, shortcut, bias: by the step itself
    assert bool((d != 0).any(0).all())
    if kernel == "mlp":
        u, W1 = fx["u"], fx["W1"]
        assert bool((u > 0).any(0).all()) and bool((u < 0).any(0).all()) and bool((u == 0).any(0).all())
        assert bool((x != 0).any(0).all()) and bool((W1 != 0).any(0).all()) and bool((W1 != 0).any(1).all())
        # b1[n] + 8 moves h[:, n] in every row with u >= 0; W1[n, k] + 8 moves u[:, n] by 8 x[:, k] and h where the old or the new
        # u is positive: for every (n, k) there is such a row
        up, xn, xp = (u >= 0).double(), (x < 0).double(), (x > 0).double()
        assert bool((up.sum(0) > 0).all())
        # rows with x[r, k] > 0 and u[r, n] >= 0 (then u + 8 x > 0), or x[r, k] < 0 and u[r, n] > 0
        reach = up.T @ xp + (u > 0).double().T @ xn
        assert bool((reach > 0).all())


SAMPLED = [("proj", 64, 3, 33), ("proj", 128, 0, 33), ("mlp", 64, 0, 40), ("mlp", 128, 3, 40), ("linear_ln", 128, 0, 33), ("linear_ln", 160, 3, 33),
           ("linear_ln", 1024, 3, 65), ("patch_embed", (3, 12, 64), 3, 27), ("patch_embed", (3, 12, 96), 0, 27), ("patch_embed", (3, 12, 128), 3, 27)]


@pytest.mark.parametrize("kernel,key,mu,M", SAMPLED)
def test_one_lattice_step_changes_the_expected_output(kernel, key, mu, M):
    """the bite check by recomputation: the weights are the master's, the rows a prefix as the GPU test runs it; 256 elements of
    every large operand and all of the small ones"""
    fx = T.take_rows(master(kernel, key, mu), M)
    ref = T.reference_out(fx)
    # the fp64 reference of the unmoved fixture is the exact expectation up to the roundings the GPU test allows
    rho = fx["rho"].float()
    assert float((T.expected_out(fx, rho).double() - ref).abs().max()) < 1e-4
    assert not T.visible(fx, ref, ref)
    g = gen(77)
    names = ["W", "b", "gamma", "beta"] + (["W1", "b1"] if kernel == "mlp" else []) + (["sc"] if kernel != "patch_embed" else [])
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # thousands of tiny products: a thread pool only gets in the way
    try:
        for name in names:
            v = fx[name]
            stepped = T.lattice_step(name, v.flatten()).view_as(v)
            n = v.numel()
            idx = torch.arange(n) if n <= 512 else torch.randperm(n, generator=g)[:256]
            for i in idx.tolist():
                moved = v.clone()
                moved.view(-1)[i] = stepped.view(-1)[i]
                assert T.visible(fx, ref, T.reference_out(fx, **{name: moved})), (name, i)
    finally:
        torch.set_num_threads(threads)


# ---- Level 2 -------------------------------------------------------------------------------------------------------------------
RANDN = [("proj", 64), ("proj", 128), ("mlp", 64), ("mlp", 128), ("linear_ln", 160), ("linear_ln", 1024), ("patch_embed", (5, 28, 96)),
         ("mlp_sweep", 64), ("mlp_sweep", 128)]


def randn_case(kernel, key):
    if kernel == "mlp_sweep":
        return T.mlp_sweep(key)
    return {"proj": T.proj_randn, "mlp": T.mlp_randn, "linear_ln": T.linln_randn}[kernel](key) if kernel != "patch_embed" else T.embed_randn(*key)


def delta_y(fx):
    if fx["kernel"] == "proj":
        return T.dy_plain(fx["C"], fx["x"].abs() @ fx["W"].abs().T + fx["b"].abs()[None])
    return fx["dy"]


@pytest.mark.parametrize("kernel,key", RANDN)
def test_norm_push_against_worst_case_perturbations(kernel, key):
    fx = randn_case(kernel, key)
    y, C = fx["y"], fx["C"]
    dy = delta_y(fx)
    assert bool((dy > 0).all())
    xh, r, bound = T.norm_push(y, dy, C)
    g = gen(5)
    M = y.shape[0]
    worst = 0.0
    for _ in range(64):
        row, c = int(torch.randint(0, M, (1,), generator=g)), int(torch.randint(0, C, (1,), generator=g))
        coef = -(1.0 + xh[row, c] * xh[row]) / C  # d xhat_c / d y_j over r
        coef[c] += 1.0
        for sign in (1.0, -1.0):
            yp = y[row] + sign * torch.sign(coef) * dy[row]
            dp = yp - yp.mean()
            got = float((dp * (dp.pow(2).mean() + T.EPS).rsqrt())[c] - xh[row, c])
            assert abs(got) <= float(bound[row, c]), (row, c, got, float(bound[row, c]))
            worst = max(worst, abs(got) / float(bound[row, c]))
    assert worst > 0.5, worst  # the bound is within a factor of two of what a perturbation inside delta_y can do
    # random sign patterns, all rows at once
    for s in range(4):
        sg = torch.randint(0, 2, y.shape, generator=g).double() * 2 - 1
        yp = y + sg * dy
        dp = yp - yp.mean(-1, keepdim=True)
        assert bool(((dp * (dp.pow(2).mean(-1, keepdim=True) + T.EPS).rsqrt() - xh).abs() <= bound).all())


@pytest.mark.parametrize("kernel,key", RANDN)
def test_a_shifted_parameter_index_leaves_the_bound(kernel, key):
    fx = randn_case(kernel, key)
    ref = T.reference_randn(fx)
    assert float((ref - fx["ref"]).abs().max()) < 1e-12
    assert bool((fx["bound"] > 0).all()) and bool((fx["bound_t"] > fx["bound"]).all())
    for name in ("gamma", "beta", "b") + (("b1",) if kernel.startswith("mlp") else ()):
        moved = T.reference_randn(fx, **{name: torch.roll(fx[name], 1)})
        out = ((moved - ref).abs() > 2 * fx["bound_t"])
        assert float(out.double().mean()) > (0.25 if name in ("gamma", "beta") else 0.0), (name, float(out.double().mean()))
    if kernel == "mlp":  # the rows: dense below 5, a few up to 40
        u = fx["u"].abs()
        hist = torch.histc(fx["u"].flatten(), bins=40, min=-5.0, max=5.0)
        assert float(hist.min()) > 100 and 25.0 < float(u.max()) < 64.0


@pytest.mark.parametrize("C", [64, 128])
def test_gelu_sweep_is_dense_exact_and_sees_a_wrong_interval(C):
    fx = T.mlp_sweep(C)
    x, u, W2 = fx["x"], fx["u"], fx["W"]
    assert bf16_exact(x) and bf16_exact(fx["W1"]) and bf16_exact(W2) and f32_exact(fx["b1"]) and f32_exact(u)
    assert bool(((fx["W1"] != 0).sum(1) == 1).all()) and bool(((W2 != 0).sum(1) <= 1).all())  # one product per sum: u and y = h exact
    seen = u[:, fx["listens"]]
    assert torch.equal(fx["y"][:, :C // 2], fx["h"][:, fx["listens"]])
    grid = torch.unique(seen)
    assert float(grid.min()) == -6.0 and float(grid.max()) > 5.9 and float((grid[1:] - grid[:-1]).max()) == 1.0 / 64
    # where the polynomial works the bound is a few 1e-4 of a pre-norm row of spread ~ 0.7
    neg = (seen > -5.0) & (seen < -1.0)
    assert float(fx["dy"][:, :C // 2][neg].max()) < 1e-3
    # the hidden unit wrong by 2.5e-3 on [-2, -1.9) or by 1e-3 on [-4.1, -4): some output leaves its bound
    for lo, hi, e in ((-2.0, -1.9, 2.5e-3), (-4.1, -4.0, 1e-3), (0.5, 0.6, 1e-2)):
        h = fx["h"] + e * ((u >= lo) & (u < hi)).double()
        y = h @ W2.T + fx["b"][None]
        d = y - y.mean(-1, keepdim=True)
        moved = d * (d.pow(2).mean(-1, keepdim=True) + T.EPS).rsqrt() * fx["gamma"][None] + fx["beta"][None] + fx["sc"]
        assert bool(((moved - fx["ref"]).abs() > fx["bound"]).any()), (lo, hi, e)
