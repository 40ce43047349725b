"""Gradient-norm clipping on the GPU: the kernels of csrc/grad_clip.hip through ops.grad_norm / ops.grad_clip against the exact
reference of tests/grad_clip_ref.py, then optim.clip_grad_norm_ / grad_norms on the tiny models.

Tolerances.  Integer-valued and power-of-two gradients: every square, every partial sum and the total S are exactly
representable in float64 whatever the order of summation, so the norms must EQUAL float32(sqrt(S)).  randn: the float64
summation error is at most n * 2^-53 relative (n <= 2^28), halved by the square root, i.e. far inside half a float32 ulp,
plus the one rounding to float32: within 1 float32 ulp of float32(sqrt(fsum of the exact squares)).  Max-abs is exact always.
Scaled gradients are one fp32 multiplication: bit-equal to g * coef with the coefficient the kernel stored."""
import math
import types

import numpy as np
import pytest
import torch

from tests import grad_clip_ref as R
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

SENT = 12345.0     # around every gradient tensor
PSENT = -7.0       # behind the used partials
RSENT = -3.0       # behind norms[nt] (and the coefficient)


def chunk():
    from klab_multimodalmodel_amd import ops
    return ops.grad_norm_chunk()


def lens9():
    c = chunk()
    return [1, 3, 4, 5, 1021, c - 1, c, c + 1, 2 * c + 3]


class Table:
    """gradient tensors inside ONE sentinel-filled buffer, each 16-byte aligned (or, for the indices in `skew`, 4 bytes past
    that) with at least four sentinel words on either side; the table, partials and result words of one klab_grad_norm call"""

    def __init__(self, arrays, skew=()):
        from klab_multimodalmodel_amd import ops
        self.ops = ops
        self.arrays = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in arrays]
        offs, o = [], 4
        for i, a in enumerate(self.arrays):
            o = (o + 3) & ~3
            if i in skew:
                o += 1
            offs.append(o)
            o += a.size + 4
        host = np.full(o + 4, SENT, dtype=np.float32)
        self.mask = np.ones(o + 4, dtype=bool)  # True = sentinel
        for off, a in zip(offs, self.arrays):
            host[off:off + a.size] = a
            self.mask[off:off + a.size] = False
        self.buf = torch.from_numpy(host).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[off:off + a.size] for off, a in zip(offs, self.arrays)]
        for i, v in enumerate(self.views):
            assert (v.data_ptr() % 16 == 4) == (i in skew)
        self.nt = len(self.arrays)
        self.desc, self.nparts = ops.grad_table(self.views)
        self.parts = torch.full((self.nparts + 8,), PSENT, dtype=torch.float64, device="cuda")
        self.res = torch.full((self.nt + 2 + 8,), RSENT, dtype=torch.float32, device="cuda")

    def norm(self, kind=0):
        self.ops.grad_norm(self.desc, self.parts, self.res, kind=kind, nparts=self.nparts)
        torch.cuda.synchronize()
        res = self.res.cpu().numpy()
        return res[:self.nt].copy(), res[self.nt].copy()

    def clip(self, max_norm):
        self.ops.grad_clip(self.desc, self.res[self.nt:self.nt + 1], max_norm, self.res[self.nt + 1:self.nt + 2])
        torch.cuda.synchronize()
        return self.res.cpu().numpy()[self.nt + 1].copy()

    def grads(self):
        h = self.buf.cpu().numpy()
        out, o = [], 0
        for v, a in zip(self.views, self.arrays):
            off = (v.data_ptr() - self.buf.data_ptr()) // 4
            out.append(h[off:off + a.size].copy())
        return out

    def check_sentinels(self, coef_written=False):
        h = self.buf.cpu().numpy()
        assert np.all(h[self.mask] == np.float32(SENT)), "a store outside a gradient tensor's extent"
        assert bool((self.parts[self.nparts:] == PSENT).all()), "a partial behind the table's count was written"
        tail = self.nt + 2 if coef_written else self.nt + 1
        assert bool((self.res[tail:] == RSENT).all()), "a result word behind norms[nt] was written"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def int_arrays(lens, seed):
    """small integers; every third tensor of a table (and a short lone one) is a 3-4-5 pattern (S = 25 k^2, a perfect square), the
    others are almost never one"""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(lens):
        if i % 3 == 0 and (len(lens) > 1 or n <= 5):
            a = np.zeros(n, dtype=np.float32)
            a[0] = 3 * (i + 1)
            if n > 1:
                a[-1] = -4 * (i + 1)
        else:
            a = rng.integers(-9, 10, size=n).astype(np.float32)
            a[0] = 7  # never all zero
        out.append(a)
    return out


def pow2_arrays(lens, seed):
    """+-2^60, +-2^64, +-2^70: squares up to 2^140, every partial sum a multiple of 2^120 below 2^173 -- exact in float64, infinite in fp32"""
    rng = np.random.default_rng(seed)
    return [(rng.choice([2.0 ** 60, 2.0 ** 64, 2.0 ** 70], size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32) for n in lens]


def randn_arrays(lens, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3)).astype(np.float32) for n in lens]


def exact_norm32(arrays):
    """float32(sqrt(S)) with S from integer arithmetic (the arrays hold integers or powers of two)"""
    s = sum(int(x) ** 2 for a in arrays for x in a.astype(np.float64).tolist())
    f = float(s)
    assert int(f) == s, "the test's own data: S must be exactly representable"
    return np.float32(np.sqrt(np.float64(f)))


def tables():
    """(name, lengths, skewed indices): 1, 2 and 9 tensors over every boundary length, and 1025 tensors (the table no longer fits LDS)"""
    L = lens9()
    out = [(f"one-{n}", [n], ()) for n in L]
    out += [("two-a", [L[7], L[3]], ()), ("two-b", [L[1], L[8]], ()), ("nine", L, ()), ("nine-skewed", L, (0, 2, 4, 5, 7, 8)),
            ("one-skewed", [L[8]], (0,)), ("many", [1 + i % 9 for i in range(1025)], ())]
    return out


TABLE_NAMES = ["one-1", "one-3", "one-4", "one-5", "one-1021", "one-c-1", "one-c", "one-c+1", "one-2c+3", "two-a", "two-b", "nine",
               "nine-skewed", "one-skewed", "many"]


@pytest.fixture(scope="module", params=range(len(TABLE_NAMES)), ids=TABLE_NAMES)
def case(request):
    name, lens, skew = tables()[request.param]
    return name, lens, skew


def test_integer_gradients_exact(case):
    name, lens, skew = case
    arrays = int_arrays(lens, 11)
    t = Table(arrays, skew)
    per, total = t.norm(0)
    want = [exact_norm32([a]) for a in arrays]
    assert same_bits(per, np.array(want)), name
    assert same_bits(total, exact_norm32(arrays)), name
    squares = sum(float(w) == int(float(w)) for w in want)
    if len(lens) >= 9:
        assert 1 <= squares < len(lens)  # some norms are integers (S a perfect square) and some are not
    mper, mtotal = t.norm(1)
    assert same_bits(mper, np.array([np.abs(a).max() for a in arrays])) and same_bits(mtotal, max(np.abs(a).max() for a in arrays))
    t.check_sentinels()
    assert all(same_bits(g, a) for g, a in zip(t.grads(), arrays))  # the norm reads only


def test_powers_of_two_finite_and_exact(case):
    name, lens, skew = case
    arrays = pow2_arrays(lens, 12)
    t = Table(arrays, skew)
    per, total = t.norm(0)
    assert np.isfinite(total) and np.all(np.isfinite(per))
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(arrays[0][0]) * np.float32(arrays[0][0]))  # where fp32 squares overflow
    assert same_bits(per, np.array([exact_norm32([a]) for a in arrays])), name
    assert same_bits(total, exact_norm32(arrays)), name
    mper, mtotal = t.norm(1)
    assert same_bits(mper, np.array([np.abs(a).max() for a in arrays])) and same_bits(mtotal, max(np.abs(a).max() for a in arrays))
    t.check_sentinels()


def test_randn_within_one_ulp_and_bit_reproducible(case):
    name, lens, skew = case
    arrays = randn_arrays(lens, 13)
    t = Table(arrays, skew)
    per, total = t.norm(0)
    parts0, res0 = t.parts.clone(), t.res.clone()
    wper, wtotal = R.norms(arrays, 2.0)
    worst = 0.0
    for g, w in zip(list(per) + [total], wper + [wtotal]):
        worst = max(worst, abs(float(g) - float(np.float32(w))) / R.ulp32(w))
        assert R.within_ulps(g, w, 1), (name, g, w)
    print(f"{name}: worst distance to float32(sqrt(fsum)) {worst:.2f} ulp over {len(lens) + 1} norms")
    per2, total2 = t.norm(0)
    assert torch.equal(parts0.view(torch.int64), t.parts.view(torch.int64)) and torch.equal(res0.view(torch.int32), t.res.view(torch.int32))
    mper, mtotal = t.norm(1)
    m2 = t.res.clone()
    t.norm(1)
    assert torch.equal(m2.view(torch.int32), t.res.view(torch.int32))
    assert same_bits(mper, np.array([np.abs(a).max() for a in arrays])) and same_bits(mtotal, max(np.abs(a).max() for a in arrays))
    t.check_sentinels()


@pytest.mark.parametrize("kind", [0, 1])
def test_nan_first_last_and_mid_chunk(kind):
    """fmax would drop a NaN: the max-abs path must keep it; so must the sum.  Only the NaN's tensor and the total are NaN."""
    c = chunk()
    lens = [5, 2 * c + 3, c + 1, 1021]
    for skew in ((), (1, 2)):
        for ti, pos in ((1, 0), (1, 2 * c + 2), (1, c + c // 2 + 1), (2, c), (0, 4), (3, 1020)):
            arrays = randn_arrays(lens, 14)
            arrays[ti][pos] = np.nan
            t = Table(arrays, skew)
            per, total = t.norm(kind)
            assert np.isnan(total), (skew, ti, pos)
            for i in range(len(lens)):
                assert np.isnan(per[i]) == (i == ti), (skew, ti, pos, i)
            t.check_sentinels()
    # an infinite gradient: an infinite norm of its tensor and of all, no NaN
    arrays = randn_arrays(lens, 15)
    arrays[1][c + 7] = -np.inf
    per, total = Table(arrays).norm(kind)
    assert np.isposinf(total) and np.isposinf(per[1]) and np.all(np.isfinite(per[[0, 2, 3]]))


def test_clip_scales_bit_exactly(case):
    name, lens, skew = case
    arrays = randn_arrays(lens, 16)
    t = Table(arrays, skew)
    _per, total = t.norm(0)
    max_norm = 0.5 * float(total)
    coef = t.clip(max_norm)
    want = R.coef(total, max_norm)  # from the kernel's own norms[nt]
    assert coef < 1 and R.within_ulps(coef, want, 1), (name, coef, want)
    for g, w in zip(t.grads(), R.scaled(arrays, coef)):
        assert same_bits(g, w), name
    t.check_sentinels(coef_written=True)
    assert same_bits(t.res.cpu().numpy()[t.nt], total)  # the clip reads the total, it does not touch it


def test_clip_above_the_norm_changes_no_bit(case):
    name, lens, skew = case
    arrays = randn_arrays(lens, 17)
    t = Table(arrays, skew)
    _per, total = t.norm(0)
    for max_norm in (float(total) * 1.5, float(total) + 1.0, 3e38, math.inf):
        coef = t.clip(max_norm)
        assert float(coef) == 1.0, (name, max_norm, coef)
        assert all(same_bits(g, a) for g, a in zip(t.grads(), arrays)), (name, max_norm)
    t.check_sentinels(coef_written=True)


@pytest.mark.parametrize("kind", [0, 1])
def test_clip_with_nonfinite_totals_as_the_reference(kind):
    c = chunk()
    lens = [5, c + 1, 1021]
    for bad, skew in ((np.nan, ()), (np.inf, ()), (-np.inf, (1,)), (np.nan, (0, 2))):
        arrays = randn_arrays(lens, 18)
        arrays[1][c - 1] = bad
        t = Table(arrays, skew)
        _per, total = t.norm(kind)
        coef = t.clip(1.0)
        wtotal, wcoef, wgrads = R.clip(arrays, 1.0, 2.0 if kind == 0 else math.inf)
        assert same_bits(total, np.float32(wtotal)) or (np.isnan(total) and math.isnan(wtotal))
        got = t.grads()
        if np.isnan(bad):
            assert np.isnan(coef) and np.isnan(wcoef)
            assert all(np.all(np.isnan(g)) for g in got)  # every gradient of every tensor
        else:
            assert float(coef) == 0.0 == float(wcoef)
            for g, w in zip(got, wgrads):
                assert same_bits(g, w)  # finite -> (signed) zero, inf * 0 -> NaN
            assert np.isnan(got[1][c - 1]) and np.count_nonzero(np.isnan(got[1])) == 1
        t.check_sentinels(coef_written=True)


def test_bad_arguments():
    from klab_multimodalmodel_amd import _lib as L
    lib = L.load()
    t = Table(randn_arrays([5, 2 * chunk() + 3], 19))
    assert t.nparts == 4
    s = L.stream_ptr()
    a = (t.desc.data_ptr(), 2)
    assert lib.klab_grad_norm(*a, 2, t.parts.data_ptr(), 4, t.res.data_ptr(), s) == L.ERR_BADARG     # kind
    assert lib.klab_grad_norm(*a, 0, t.parts.data_ptr(), 1, t.res.data_ptr(), s) == L.ERR_BADARG     # fewer partials than tensors
    assert lib.klab_grad_norm(*a, 0, None, 4, t.res.data_ptr(), s) == L.ERR_BADARG
    assert lib.klab_grad_norm(*a, 0, t.parts.data_ptr(), 4, None, s) == L.ERR_BADARG
    assert lib.klab_grad_norm(None, 2, 0, t.parts.data_ptr(), 4, t.res.data_ptr(), s) == L.ERR_BADARG
    assert lib.klab_grad_norm(t.desc.data_ptr(), -1, 0, t.parts.data_ptr(), 4, t.res.data_ptr(), s) == L.ERR_BADARG
    assert lib.klab_grad_clip(*a, None, 1.0, t.res.data_ptr(), s) == L.ERR_BADARG
    assert lib.klab_grad_clip(*a, t.res.data_ptr(), 1.0, None, s) == L.ERR_BADARG
    assert lib.klab_grad_clip(*a, t.res.data_ptr(), 1.0, t.res.data_ptr(), s) == L.ERR_BADARG
    with pytest.raises(ValueError, match="needs 4 partials"):  # the wrapper knows the exact count
        t.ops.grad_norm(t.desc, t.parts[:3], t.res, nparts=t.nparts)
    torch.cuda.synchronize()
    t.check_sentinels()  # nothing ran
    assert bool((t.res == RSENT).all())
    # no tensors at all: a total of 0
    assert lib.klab_grad_norm(None, 0, 0, None, 0, t.res.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert float(t.res[0]) == 0.0 and bool((t.res[1:] == RSENT).all())


# ---- the optimizer-side functions on the tiny models ----------------------------------------------------------------------------------
def build(train_swin=False, dtype=torch.float32):
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_golden("tiny_a")
    sw, t5 = SwinConfig.from_dict(g["meta"]["swin_config"]), T5Config.from_dict(g["meta"]["t5_config"])
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=train_swin,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], g["sds"]["main"]), dtype=dtype).to("cuda")
    m._direct_grads = True
    m.transformer.eval()
    return m, g


def fwd_bwd(m, g):
    inp = g["inputs"]  # B = 2: the first two rows of the golden batch
    loss = m({"pixel_values": inp["pixel_values"][:2].cuda()}, {"input_ids": inp["src_ids"][:2].cuda()}, {"input_ids": inp["tgt_ids"][:2].cuda()})
    loss.backward()
    return loss


def host_grads(params):
    return [p.grad.detach().cpu().numpy().copy() for p in params if p.grad is not None]


def stored_coef(params):
    """the coefficient the last clip of exactly these gradients stored (the cached state of their table)"""
    from klab_multimodalmodel_amd import optim
    params = [p for p in params if p.grad is not None]
    st, _owner = optim._clip_native(params, [p.grad for p in params], 2.0)
    return np.float32(st.res[st.nt + 1].item())


def test_model_clip_then_fused_adam_and_second_call():
    from klab_multimodalmodel_amd import optim
    m, g = build()
    opt = optim.FusedAdam(m.transformer.parameters(), lr=1e-3)
    fwd_bwd(m, g)
    params = list(m.transformer.parameters())
    before = host_grads(params)
    ptrs = [p.grad.data_ptr() for p in params]
    _per, want_total = R.norms(before, 2.0)
    max_norm = 0.5 * want_total
    optim.grad_norms(params)  # builds the table of these gradients (an upload); nothing is scaled
    torch.cuda.set_sync_debug_mode("error")  # no host read inside
    try:
        total = optim.clip_grad_norm_(m.transformer.parameters(), max_norm)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert total.dim() == 0 and total.dtype == torch.float32 and total.device == params[0].device
    assert R.within_ulps(total.item(), want_total, 1), (total.item(), want_total)
    coef = stored_coef(params)
    assert coef < 1 and R.within_ulps(coef, R.coef(total.item(), max_norm), 1)
    for p, b, ptr in zip(params, before, ptrs):
        assert p.grad.data_ptr() == ptr
        assert same_bits(p.grad.cpu().numpy(), b * coef)
    opt.step()
    assert opt._fallback is None and opt._fb_reason is None, opt._fb_reason
    # a second call, far above the norm: no bit changes (step() leaves the gradients where they are)
    after = host_grads(params)
    total2 = optim.clip_grad_norm_(params, 1e30)
    assert R.within_ulps(total2.item(), R.norms(after, 2.0)[1], 1)
    assert all(same_bits(a, b) for a, b in zip(host_grads(params), after))
    # max-abs, clipped
    want_inf = R.norms(after, math.inf)[1]
    tinf = optim.clip_grad_norm_(params, 0.25 * want_inf, norm_type="inf")
    assert same_bits(tinf.item(), want_inf)
    cinf = stored_coef(params)
    assert R.within_ulps(cinf, R.coef(tinf.item(), 0.25 * want_inf), 1)
    assert all(same_bits(a, b * cinf) for a, b in zip(host_grads(params), after))
    # error_if_nonfinite: torch's message
    with torch.no_grad():
        params[3].grad.view(-1)[0] = float("nan")
    with pytest.raises(RuntimeError, match="is non-finite, so it cannot be clipped"):
        optim.clip_grad_norm_(params, 1.0, error_if_nonfinite=True)


def test_model_clip_then_fused_adafactor():
    from klab_multimodalmodel_amd import optim
    m, g = build()
    opt = optim.FusedAdafactor(m.transformer.parameters())
    fwd_bwd(m, g)
    params = list(m.transformer.parameters())
    before = host_grads(params)
    want_total = R.norms(before, 2.0)[1]
    total = optim.clip_grad_norm_(params, 0.5 * want_total)
    assert R.within_ulps(total.item(), want_total, 1)
    coef = stored_coef(params)
    assert R.within_ulps(coef, R.coef(total.item(), 0.5 * want_total), 1)
    assert all(same_bits(p.grad.cpu().numpy(), b * coef) for p, b in zip(params, before))
    opt.step()
    assert opt._flat_live and opt._fb_reason is None, opt._fb_reason


def test_model_with_trainable_swin_covers_both_flat_buffers_and_names():
    from klab_multimodalmodel_amd import optim
    m, g = build(train_swin=True)
    fwd_bwd(m, g)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad and p.grad is not None]
    assert any(n.startswith("image_model.") for n, _p in named) and any(n.startswith("transformer.") for n, _p in named)
    assert all(p.grad is None for p in m.language_model.parameters())
    flats = {m.flat_grads("main").data_ptr(): m.flat_grads("main"), m.flat_grads("swin").data_ptr(): m.flat_grads("swin")}
    used = set()
    for _n, p in named:  # both flat buffers hold gradients of the list
        for base, f in flats.items():
            if base <= p.grad.data_ptr() < base + 4 * f.numel():
                used.add(base)
    assert len(used) == 2
    before = host_grads([p for _n, p in named])
    wper, wtotal = R.norms(before, 2.0)
    # per-parameter norms first (nothing is scaled by them)
    names, norms = m.grad_norms()
    order = [k for k in m.state_dict() if k in dict(named)]
    assert names == [n for n, _p in named] == order
    assert norms.dtype == torch.float32 and norms.shape == (len(named) + 1,) and norms.is_cuda
    h = norms.cpu().numpy()
    for n, a, w in zip(names, h[:-1], wper):
        assert R.within_ulps(a, w, 1), (n, a, w)
    assert R.within_ulps(h[-1], wtotal, 1)
    inames, inorms = m.grad_norms(norm_type=math.inf)
    assert inames == names and same_bits(inorms.cpu().numpy(), np.array(R.norms(before, math.inf)[0] + [R.norms(before, math.inf)[1]]))
    # the whole model's parameters: frozen ones (no gradient) are skipped
    total = optim.clip_grad_norm_(m.parameters(), 0.5 * wtotal)
    assert same_bits(total.item(), h[-1])
    coef = stored_coef([p for _n, p in named])
    assert R.within_ulps(coef, R.coef(total.item(), 0.5 * wtotal), 1)
    for (n, p), b in zip(named, before):
        assert same_bits(p.grad.cpu().numpy(), b * coef), n
    # indices for anything that is not a model
    idx, _ = optim.grad_norms(list(m.parameters()))
    assert idx == [i for i, p in enumerate(m.parameters()) if p.grad is not None]


def test_step_in_backward_is_refused():
    from klab_multimodalmodel_amd import optim
    m, g = build()
    opt = optim.FusedAdam(m.transformer.parameters(), lr=1e-3, step_in_backward=True)
    fwd_bwd(m, g)
    optim.clip_grad_norm_(m.transformer.parameters(), 1.0)  # the first step runs the ordinary way: nothing is updated yet
    opt.step()
    opt.zero_grad()
    fwd_bwd(m, g)
    assert opt.in_backward_updates == 1
    with pytest.raises(RuntimeError, match="step_in_backward=False"):
        optim.clip_grad_norm_(m.transformer.parameters(), 1.0)
    opt.step()  # joins the side stream
    torch.cuda.synchronize()
    assert opt._fallback is None


def test_bf16_gradient_delegates_to_torch():
    from klab_multimodalmodel_amd import optim

    def make():
        gen = torch.Generator().manual_seed(5)
        ps = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in ((33, 7), (1021,), (5,))]
        ps[1].data = ps[1].data.bfloat16()
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen).to(p.device, p.dtype)
        return ps
    a, b = make(), make()
    ra, rb = optim.clip_grad_norm_(a, 0.5), torch.nn.utils.clip_grad_norm_(b, 0.5)
    assert torch.equal(ra, rb)
    assert all(p.grad.dtype == q.grad.dtype and torch.equal(p.grad, q.grad) for p, q in zip(a, b))
    with pytest.raises(NotImplementedError):
        optim.grad_norms(a)


def test_foreign_fp32_gradients_take_the_native_path():
    """parameters no klab model owns: keyed on (data_ptr, numel), finite where torch's fp32 squares overflow"""
    from klab_multimodalmodel_amd import optim
    ps = [torch.nn.Parameter(torch.zeros(n, device="cuda")) for n in (7, 1021, 70000)]
    arrays = pow2_arrays([7, 1021, 70000], 21)
    for p, a in zip(ps, arrays):
        p.grad = torch.from_numpy(a).cuda()
    assert math.isinf(float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in ps]))))
    optim._CLIP_CACHE.clear()
    total = optim.clip_grad_norm_(ps, 1.0)
    assert len(optim._CLIP_CACHE) == 1
    assert same_bits(total.item(), exact_norm32(arrays)) and math.isfinite(total.item())
    coef = stored_coef(ps)
    assert R.within_ulps(coef, R.coef(total.item(), 1.0), 1)
    assert all(same_bits(p.grad.cpu().numpy(), a * coef) for p, a in zip(ps, arrays))
    optim.clip_grad_norm_(ps, 1.0)
    assert len(optim._CLIP_CACHE) == 1  # the same tensors: the cached table
    names, norms = optim.grad_norms(ps)
    assert names == [0, 1, 2] and norms.shape == (4,)
