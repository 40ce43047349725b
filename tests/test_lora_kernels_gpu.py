"""The two LoRA kernels on the GPU through ops (klab_lora_merge, klab_lora_grads) against the fp64 statements and the per-element
bounds of tests/lora_ref.py (proved on three f32 orders in tests/test_lora_cpu.py): tables of 1 and 7 tensors of mixed shapes that are
no multiple of the 64 x 64 tile and end in partial row blocks, ranks 1, 3, 8, 16 and 64, bf16 and f32 arenas.  Bit-exact on the
integer fixtures, inside the bound for every element on the randn fixtures; sentinels around every tensor, inputs and everything no
table entry names keep their bits."""
import pytest
import torch

from tests import lora_ref as R
from tests.adamw_ref import bits

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float32)
SENT = -123.5


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


class Dev:
    """a fixture's tensors on the device and its table"""

    def __init__(self, ops, f):
        self.f = f
        self.W, self.A, self.B = ([t.cuda() for t in ts] for ts in (f.W, f.A, f.B))
        self.desc, self.plan, self.n_out, self.n_slab = ops.lora_table(
            [(w, a, b, ao, go, f.s) for w, a, b, ao, go in zip(self.W, self.A, self.B, f.aoff, f.goff)])
        assert tuple(self.desc.shape) == (f.n, 11)

    def inputs_unchanged(self, w_too=True):
        f = self.f
        for mine, theirs in ((self.A, f.A), (self.B, f.B)) + (((self.W, f.W),) if w_too else ()):
            assert all(torch.equal(bits(a.cpu()), bits(b)) for a, b in zip(mine, theirs))


def merge(ops, f, dtype):
    """one klab_lora_merge into an arena of `dtype` -> (the arena on the host, the device side)"""
    d = Dev(ops, f)
    arena = f.arena(dtype).cuda()
    try:
        ops.lora_merge(d.desc, arena)
    finally:
        torch.cuda.synchronize()
    out = arena.cpu()
    d.inputs_unchanged()
    keep = ~f.arena_mask()  # the sentinels around every tensor, and the arena tensor no entry names
    assert torch.equal(bits(out[keep]), bits(f.arena(dtype)[keep]))
    return out, d


def tensors_of(f, arena):
    return [arena[ao:ao + o * i].view(o, i) for (o, i), ao in zip(f.shapes, f.aoff)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", R.RANKS)
@pytest.mark.parametrize("n", R.NTAB)
def test_merge_is_bit_exact_on_the_integer_fixtures(ops, n, r, dtype):
    f = R.Fixture(n, r, "int")
    out, _d = merge(ops, f, dtype)
    for got, W, A, B in zip(tensors_of(f, out), f.W, f.A, f.B):
        exact = R.merge_ref(W, A, B, f.s, dtype)[0]
        assert torch.equal(bits(got), bits(exact.to(dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", R.RANKS)
@pytest.mark.parametrize("n", R.NTAB)
def test_merge_is_within_the_bound_for_every_element_and_moves_what_must_move(ops, n, r, dtype):
    f = R.Fixture(n, r, "randn")
    out, _d = merge(ops, f, dtype)
    worst = 0.0
    for got, W, A, B in zip(tensors_of(f, out), f.W, f.A, f.B):
        exact, bound = R.merge_ref(W, A, B, f.s, dtype)
        worst = max(worst, R.worst(got, exact, bound))
        mv = R.must_move(W, A, B, f.s, dtype)
        assert bool((got[mv] != W.to(dtype)[mv]).all())
    print(f"lora merge n={n} r={r} {dtype}: err / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("r", (3, 64))
@pytest.mark.parametrize("n", R.NTAB)
def test_to_master_writes_the_f32_value_whose_cast_the_arena_holds(ops, n, r):
    f = R.Fixture(n, r, "randn")
    a16, _d = merge(ops, f, torch.bfloat16)
    a32, _d = merge(ops, f, torch.float32)
    d = Dev(ops, f)
    try:
        ops.lora_merge(d.desc, to_master=True)
    finally:
        torch.cuda.synchronize()
    d.inputs_unchanged(w_too=False)
    for w, g16, g32, W in zip(d.W, tensors_of(f, a16), tensors_of(f, a32), f.W):
        w = w.cpu()
        assert torch.equal(bits(w), bits(g32)) and torch.equal(bits(w.to(torch.bfloat16)), bits(g16))
        assert not torch.equal(w, W)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", (1, 8, 64))
def test_merge_with_b_zero_is_torchs_own_cast(ops, r, dtype):
    f = R.Fixture(7, r, "randn", b_zero=True)
    out, _d = merge(ops, f, dtype)
    for got, W in zip(tensors_of(f, out), f.W):
        assert torch.equal(bits(got), bits(W.to(dtype)))


def test_table_limits_and_bad_arguments(ops):
    from klab_multimodalmodel_amd import _lib
    lib = _lib.load()
    f = R.Fixture(1, 3, "int")
    d = Dev(ops, f)
    arena = f.arena(torch.float32).cuda()
    out, slab, g = torch.zeros(d.n_out).cuda(), torch.zeros(d.n_slab).cuda(), f.grads().cuda()
    sp, p = _lib.stream_ptr(), d.desc.data_ptr()
    assert lib.klab_lora_merge(p, 1025, arena.data_ptr(), _lib.F32, 0, sp) == _lib.ERR_UNSUPPORTED  # refused on the host: no launch
    assert lib.klab_lora_grads(p, 1025, g.data_ptr(), out.data_ptr(), slab.data_ptr(), sp) == _lib.ERR_UNSUPPORTED
    assert lib.klab_lora_merge(p, 0, arena.data_ptr(), _lib.F32, 0, sp) == 0
    assert lib.klab_lora_grads(p, 0, g.data_ptr(), out.data_ptr(), slab.data_ptr(), sp) == 0
    assert lib.klab_lora_merge(None, 1, arena.data_ptr(), _lib.F32, 0, sp) == _lib.ERR_BADARG
    assert lib.klab_lora_merge(p, 1, None, _lib.F32, 0, sp) == _lib.ERR_BADARG
    assert lib.klab_lora_merge(p, 1, arena.data_ptr(), 77, 0, sp) == _lib.ERR_BADARG
    assert lib.klab_lora_merge(p, -1, arena.data_ptr(), _lib.F32, 0, sp) == _lib.ERR_BADARG
    assert lib.klab_lora_grads(p, 1, None, out.data_ptr(), slab.data_ptr(), sp) == _lib.ERR_BADARG
    assert lib.klab_lora_grads(p, 1, g.data_ptr(), None, slab.data_ptr(), sp) == _lib.ERR_BADARG
    assert lib.klab_lora_grads(p, 1, g.data_ptr(), out.data_ptr(), None, sp) == _lib.ERR_BADARG
    torch.cuda.synchronize()
    assert torch.equal(bits(arena.cpu()), bits(f.arena(torch.float32))) and float(out.abs().max()) == 0.0
    with pytest.raises(ValueError):
        ops.lora_table([(d.W[0], d.A[0][:, :-4].contiguous(), d.B[0], 0, 0, 1.0)])  # shapes that do not fit
    with pytest.raises(ValueError):
        ops.lora_table([(d.W[0], d.A[0], d.B[0], 2, 0, 1.0)])  # an arena offset that is no multiple of 4


# ---- klab_lora_grads -----------------------------------------------------------------------------------------------------------------
def grads(ops, f, d=None):
    """one klab_lora_grads over pre-filled outputs -> ([(dA, dB)] on the host, out, slab, the device side)"""
    d = d or Dev(ops, f)
    g = f.grads().cuda()
    out = torch.full((d.n_out + R.GAP,), SENT).cuda()
    slab = torch.full((d.n_slab + R.GAP,), SENT).cuda()
    try:
        ops.lora_grads(d.desc, g, out, slab)
    finally:
        torch.cuda.synchronize()
    d.inputs_unchanged()
    assert torch.equal(bits(g.cpu()), bits(f.grads()))  # dW (and the sentinels between the tensors) are only read
    out, slab = out.cpu(), slab.cpu()
    res, covered = [], torch.zeros(out.numel(), dtype=torch.bool)
    for (o, i), (n4, _rb, _so, db) in zip(f.shapes, d.plan):
        res.append((out[4 * n4:4 * n4 + f.r * i].view(f.r, i), out[db:db + o * f.r].view(o, f.r)))
        covered[4 * n4:4 * n4 + f.r * i] = True
        covered[db:db + o * f.r] = True
    assert bool((out[~covered] == SENT).all())   # the padding between the dB ranges and everything behind the last one
    assert bool((out[covered] != SENT).all())    # every output element was overwritten
    assert bool((slab[d.n_slab:] == SENT).all()) and bool((slab[:d.n_slab] != SENT).all())  # the slab: [blocks, r, in] per tensor, no more
    return res, out, slab, d


@pytest.mark.parametrize("r", R.RANKS)
@pytest.mark.parametrize("n", R.NTAB)
def test_grads_are_bit_exact_on_the_integer_fixtures(ops, n, r):
    f = R.Fixture(n, r, "int")
    res = grads(ops, f)[0]
    for (gA, gB), dW, A, B in zip(res, f.dW, f.A, f.B):
        dA, _ba, dB, _bb = R.grads_ref(dW, A, B, f.s)
        assert torch.equal(gA.double(), dA) and torch.equal(gB.double(), dB)


@pytest.mark.parametrize("r", R.RANKS)
@pytest.mark.parametrize("n", R.NTAB)
def test_grads_are_within_the_bounds_for_every_element_and_the_same_on_every_run(ops, n, r):
    f = R.Fixture(n, r, "randn")
    res, out, slab, d = grads(ops, f)
    wa = wb = 0.0
    for (gA, gB), dW, A, B in zip(res, f.dW, f.A, f.B):
        dA, bA, dB, bB = R.grads_ref(dW, A, B, f.s)
        wa, wb = max(wa, R.worst(gA, dA, bA)), max(wb, R.worst(gB, dB, bB))
    print(f"lora grads n={n} r={r}: err / bound dA {wa:.3f} dB {wb:.3f}")
    assert wa <= 1.0 and wb <= 1.0
    _res, out2, slab2, _d = grads(ops, f, d)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(slab), bits(slab2))


@pytest.mark.parametrize("r", (1, 8, 64))
def test_grads_with_b_zero_give_zero_da_and_the_right_db(ops, r):
    f = R.Fixture(7, r, "randn", b_zero=True)
    res = grads(ops, f)[0]
    worst = 0.0
    for (gA, gB), dW, A, B in zip(res, f.dW, f.A, f.B):
        assert float(gA.abs().max()) == 0.0
        _dA, _ba, dB, bB = R.grads_ref(dW, A, B, f.s)
        worst = max(worst, R.worst(gB, dB, bB))
        assert float(gB.abs().max()) > 0.0
    assert worst <= 1.0
