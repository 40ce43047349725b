"""The fused weight EMA on the GPU: klab_ema_update_range / klab_ema_swap_range through the C ABI against the fp64 reference and the
per-element bound of tests/ema_ref.py (proved on three f32 forms in tests/test_ema_cpu.py; tables in LDS, n = 5, and in global
memory, n = 1100), and optim.WeightEMA on the tiny golden model next to optim.FusedAdamW: the one-launch update and swap, the
compute-dtype copies the swap leaves, step_in_backward, re-bind, checkpoint and the torch path of a foreign module.

'Every element moved' is asked of the elements that CAN move (ema_ref.must_move): where w |p - e| is below half a spacing of e the
fp64 reference itself rounds back to e, so no correct f32 evaluation changes the element (21 of the 575056 elements of the
n = 1100 fixture with w = 2^-10, counted on the CPU for all three f32 forms); those elements are still held to the bound.

The arena copies are compared with torch's own cast bit for bit, except where that cast gives a NaN: which NaN a conversion
returns is the converter's choice (torch's CPU cast returns 0xFFFF for the planted 0x7FC01234, truncation would give 0x7FC0, and
round-to-nearest-even says nothing about it), so there the arena has to hold a NaN too, and no more is asked.  The planted
denormal lies below half the smallest bf16 denormal: it rounds to +0, and a conversion that flushes gives +0 too.  In p and in
the shadow the f32 bits of every planted value, the NaN's payload included, must survive the exchange whatever the arena's type."""
import os

import pytest
import torch

from tests import adamw_ref as A
from tests import ema_ref as E
from tests.adamw_ref import bits
from tests.engine_kernels_ref import gen, with_bf16_ties
from tests.test_adamw_gpu import build, run, train, two_groups

pytestmark = pytest.mark.gpu

NTAB = (5, 1100)  # 1100 > 1024: the descriptor table is read from global memory


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


@pytest.fixture(scope="module")
def states():
    return {n: A.AdamWState(n, seed=63) for n in NTAB}


def table(s, pd):
    return torch.tensor([[pd.data_ptr() + 4 * po, go, ao, p4] for po, go, ao, p4 in zip(s.poff, s.goff, s.aoff, s.pre)], dtype=torch.int64).cuda()


def sub_range(s):
    return (1, 4) if s.n == 5 else (s.n // 3, 2 * s.n // 3)


# ---- the update kernel through the C ABI ------------------------------------------------------------------------------------------------
def update(ops, s, w, begin4=0, end4=None):
    """one klab_ema_update_range with the fixture's m as the shadow -> (p, ema, arena) on the host"""
    pd, ed, ad = s.p.cuda(), s.m.cuda(), s.arena.cuda()
    desc = table(s, pd)
    try:
        ops.ema_update(desc, ed, w, begin4=begin4, end4=end4, total4=s.total4)
    finally:
        torch.cuda.synchronize()
        out = pd.cpu(), ed.cpu(), ad.cpu()
    return out


def assert_untouched(s, out, ema_too=False):
    p1, e1, a1 = out
    assert torch.equal(bits(p1), bits(s.p)) and torch.equal(bits(a1), bits(s.arena))  # p is only read, no arena is touched
    if ema_too:
        assert torch.equal(bits(e1), bits(s.m))


@pytest.mark.parametrize("w", E.WEIGHTS)
@pytest.mark.parametrize("n", NTAB)
def test_update_is_within_the_bound_for_every_element(ops, states, n, w):
    s = states[n]
    out = update(ops, s, w)
    assert_untouched(s, out)
    _mp, mg, _ma = s.masks(range(n))
    assert torch.equal(bits(out[1])[~mg], bits(s.m)[~mg])  # the gaps of the shadow's layout
    worst = 0.0
    for i in range(n):
        P, E0, E1 = s.p[s.poff[i]:][:s.lens[i]], s.m[s.goff[i]:][:s.lens[i]], out[1][s.goff[i]:][:s.lens[i]]
        worst = max(worst, E.worst(E1, P, E0, w))
        must = E.must_move(P, E0, w)
        assert bool((E1[must] != E0[must]).all()), i
    print(f"ema update n={n} w={w:.3e}: err / bound {worst:.3f}")
    assert worst <= 1.0
    P, E0 = s.gather(s.p, s.poff), s.gather(s.m, s.goff)
    assert float(E.must_move(P, E0, w).float().mean()) > 0.99 and bool((P != E0).all())


@pytest.mark.parametrize("n", NTAB)
def test_update_of_a_sub_range_touches_only_its_tensors(ops, states, n):
    s = states[n]
    full = update(ops, s, E.W_999)
    i0, i1 = sub_range(s)
    part = update(ops, s, E.W_999, begin4=s.pre[i0], end4=s.pre[i1])
    assert_untouched(s, part)
    _mp, mg, _ma = s.masks(range(i0, i1))
    assert torch.equal(bits(part[1])[mg], bits(full[1])[mg])   # the same update inside the range
    assert torch.equal(bits(part[1])[~mg], bits(s.m)[~mg])     # bit for bit untouched outside it
    assert not torch.equal(part[1][mg], s.m[mg])
    # an empty range: nothing is launched, nothing changes
    assert_untouched(s, update(ops, s, E.W_999, begin4=s.pre[i0], end4=s.pre[i0]), ema_too=True)


def test_update_refuses_bad_arguments_and_leaves_every_buffer(ops, states):
    from klab_multimodalmodel_amd import _lib
    s = states[5]
    for w in (1.5, float("nan"), -0.5):
        with pytest.raises(ValueError):
            update(ops, s, w)
    lib = _lib.load()
    pd, ed, ad = s.p.cuda(), s.m.cuda(), s.arena.cuda()
    desc = table(s, pd)
    sp = _lib.stream_ptr()
    assert lib.klab_ema_update_range(desc.data_ptr(), s.n, 0, s.total4, ed.data_ptr(), 1.5, sp) == _lib.ERR_BADARG
    assert lib.klab_ema_update_range(desc.data_ptr(), s.n, 0, s.total4, ed.data_ptr(), float("nan"), sp) == _lib.ERR_BADARG
    assert lib.klab_ema_update_range(desc.data_ptr(), s.n, 0, s.total4, None, 0.5, sp) == _lib.ERR_BADARG
    assert lib.klab_ema_update_range(None, s.n, 0, s.total4, ed.data_ptr(), 0.5, sp) == _lib.ERR_BADARG
    assert lib.klab_ema_update_range(desc.data_ptr(), s.n, 4, 0, ed.data_ptr(), 0.5, sp) == _lib.ERR_BADARG
    assert lib.klab_ema_swap_range(desc.data_ptr(), s.n, 0, s.total4, ed.data_ptr(), ad.data_ptr(), 77, sp) == _lib.ERR_BADARG
    assert lib.klab_ema_swap_range(desc.data_ptr(), s.n, 0, s.total4, ed.data_ptr(), None, _lib.BF16, sp) == _lib.ERR_BADARG
    torch.cuda.synchronize()
    assert_untouched(s, (pd.cpu(), ed.cpu(), ad.cpu()), ema_too=True)


# ---- the swap kernel through the C ABI --------------------------------------------------------------------------------------------------
NAN_PAYLOAD, NEG_ZERO, P_INF, N_INF, DENORMAL = 0x7FC01234, -0x80000000, 0x7F800000, -0x00800000, 0x00000005
SPECIALS = (NAN_PAYLOAD, NEG_ZERO, P_INF, N_INF, DENORMAL)


def swap_inputs(s):
    """p and a shadow with bf16 ties; NaN with a payload, -0, +-inf and a denormal planted in both, in a tensor with an arena copy
    and in one without"""
    p = s.p.clone()
    e = with_bf16_ties(s.m.clone(), gen(64))
    with_copy = next(i for i in range(s.n) if s.has_a[i] and s.lens[i] >= 16)
    without = next(i for i in range(s.n) if not s.has_a[i] and s.lens[i] >= 16)
    sp = torch.tensor(SPECIALS, dtype=torch.int32)
    for i in (with_copy, without):
        bits(p)[s.poff[i] + 1:s.poff[i] + 6] = sp
        bits(e)[s.goff[i] + 7:s.goff[i] + 12] = sp.flip(0)
    assert p[s.poff[with_copy] + 1].isnan() and e[s.goff[without] + 11].isnan()
    return p, e, (with_copy, without)


def swap(ops, s, p, e, arena, begin4=0, end4=None, twice=False):
    pd, ed, ad = p.cuda(), e.cuda(), arena.cuda()
    desc = table(s, pd)
    try:
        for _ in range(2 if twice else 1):
            ops.ema_swap(desc, ed, ad, begin4=begin4, end4=end4, total4=s.total4)
    finally:
        torch.cuda.synchronize()
        out = pd.cpu(), ed.cpu(), ad.cpu()
    return out


def assert_same_cast(got, want, what):
    """bit for bit where torch's cast is a number or an infinity; a NaN where it is a NaN"""
    nan = want.isnan()
    assert torch.equal(bits(got)[~nan], bits(want)[~nan]), what
    assert bool(got[nan].isnan().all()), what


def check_swapped(s, p, e, arena, out, tensors):
    """the listed tensors exchanged and their arena copies written; everything else bit for bit as before"""
    p1, e1, a1 = out
    mp, mg, ma = s.masks(tensors)
    for i in tensors:
        n = s.lens[i]
        assert torch.equal(bits(p1)[s.poff[i]:][:n], bits(e)[s.goff[i]:][:n]), i  # the bits of p are the old bits of ema ...
        assert torch.equal(bits(e1)[s.goff[i]:][:n], bits(p)[s.poff[i]:][:n]), i  # ... and vice versa
        if s.has_a[i]:
            assert_same_cast(a1[s.aoff[i]:][:n], p1[s.poff[i]:][:n].to(arena.dtype), i)
    assert torch.equal(bits(p1)[~mp], bits(p)[~mp]) and torch.equal(bits(e1)[~mg], bits(e)[~mg])
    assert torch.equal(bits(a1)[~ma], bits(arena)[~ma])  # tensors without a copy, the gaps, tensors outside the range


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", NTAB)
def test_swap_exchanges_the_bits_and_writes_the_arena(ops, states, n, dtype):
    s = states[n]
    p, e, (with_copy, _without) = swap_inputs(s)
    arena = torch.full((len(s.arena),), float("nan"), dtype=dtype)
    out = swap(ops, s, p, e, arena)
    check_swapped(s, p, e, arena, out, range(n))
    if dtype == torch.bfloat16:  # the ties went to even, and the planted values arrived as every conversion gives them
        ties = bits(out[0]) & 0xFFFF == 0x8000
        _mp, _mg, ma = s.masks(range(n))
        assert int(ties.sum()) > 100 and int(ma.sum()) > 0
        a = s.aoff[with_copy] + 7
        got = [int(v) & 0xFFFF for v in bits(out[2])[a:a + 5]]
        assert got[:4] == [0x0000, 0xFF80, 0x7F80, 0x8000] and got[4] & 0x7F80 == 0x7F80 and got[4] & 0x7F != 0  # ..., a NaN
    # a second swap restores p and ema bit for bit (and the arena holds the copies of p again)
    back = swap(ops, s, p, e, arena, twice=True)
    assert torch.equal(bits(back[0]), bits(p)) and torch.equal(bits(back[1]), bits(e))
    for i in range(n):
        if s.has_a[i]:
            assert_same_cast(back[2][s.aoff[i]:][:s.lens[i]], p[s.poff[i]:][:s.lens[i]].to(dtype), i)


@pytest.mark.parametrize("n", NTAB)
def test_swap_of_a_sub_range_touches_only_its_tensors(ops, states, n):
    s = states[n]
    p, e, _where = swap_inputs(s)
    i0, i1 = sub_range(s)
    out = swap(ops, s, p, e, s.arena, begin4=s.pre[i0], end4=s.pre[i1])
    check_swapped(s, p, e, s.arena, out, range(i0, i1))
    none = swap(ops, s, p, e, s.arena, begin4=s.pre[i1], end4=s.pre[i1])
    check_swapped(s, p, e, s.arena, none, range(0))


# ---- optim.WeightEMA on the tiny golden model -------------------------------------------------------------------------------------------
def offsets(m):
    m._grad_targets()
    return {id(p): v.storage_offset() for p, v, mn in m._views if mn == "main"}


def flat_of(m, tensors):
    """the listed per-parameter tensors (in the order of the trainable T5) in the layout of the flat buffers, on the host"""
    offs = offsets(m)
    out = torch.zeros(m._flat["main"].numel(), dtype=torch.float32)
    mask = torch.zeros(out.numel(), dtype=torch.bool)
    for p, t in zip(tracked(m), tensors):
        o = offs[id(p)]
        out[o:o + p.numel()] = t.detach().reshape(-1).cpu()
        mask[o:o + p.numel()] = True
    return out, mask


def tracked(m):
    return [p for _n, p in m.transformer.named_parameters() if p.requires_grad]


def shadow_flat(ema, m):
    if ema._flat is not None:
        return ema._flat.cpu()
    return flat_of(m, ema._shadow)[0]


def step_update_check(m, g, opt, ema, label, **kw):
    """one training step and one update; the shadow read before the update, the parameters read after the step"""
    loss = train(m, g, opt, 1, **kw)[0]
    e0 = shadow_flat(ema, m)
    p1, mask = flat_of(m, tracked(m))
    ema.update()
    assert ema._fb_reason is None and ema._flat is not None, ema._fb_reason
    w = E.weight_at(ema.decay, ema.warmup, ema.num_updates)
    e1 = ema._flat.cpu()
    r = E.worst(e1[mask], p1[mask], e0[mask], w)
    print(f"WeightEMA {label} update {ema.num_updates} (w = {w:.4f}): err / bound {r:.3f}")
    assert r <= 1.0
    assert torch.equal(bits(e1)[~mask], bits(e0)[~mask])
    assert torch.equal(bits(flat_of(m, tracked(m))[0]), bits(p1))  # the parameters are only read
    return loss


def eval_loss(m, g):
    with torch.no_grad():
        return float(run(m, g))


def greedy(m, g):
    inp = g["inputs"]
    return m.generate(inp["pixel_values"].cuda(), inp["src_ids"].cuda(), max_length=8).cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_weight_ema_follows_the_rule_and_swaps_with_current_copies(dtype):
    from klab_multimodalmodel_amd.optim import FusedAdamW, WeightEMA
    m, g = build("tiny_a", dtype)
    opt = FusedAdamW(two_groups(m), lr=3e-3)
    with torch.no_grad():
        run(m, g)  # binds the engine
    ema = WeightEMA(m, decay=0.999)
    for _ in range(4):
        step_update_check(m, g, opt, ema, str(dtype))
    assert ema.num_updates == 4 and ema._fb_reason is None and opt._fallback is None
    assert ema._flat.shape == m._flat["main"].shape and ema._flat.dtype == torch.float32

    raw = [p.detach().clone() for p in tracked(m)]
    avg = ema.state_dict()["shadow"]
    names = [n for n, p in m.transformer.named_parameters() if p.requires_grad]
    assert m._trainable_current()
    before = eval_loss(m, g)
    with ema.average_parameters():
        assert m._trainable_current()  # the swap left the compute-dtype copies of the averaged weights: no cast
        assert all(torch.equal(bits(p.detach()), bits(avg[n])) for n, p in zip(names, tracked(m)))
        loss_in = eval_loss(m, g)
        toks_in = greedy(m, g)
        with pytest.raises(RuntimeError, match="swapped in"):
            ema.update()
    assert all(torch.equal(bits(p.detach()), bits(r)) for p, r in zip(tracked(m), raw))
    assert m._trainable_current()
    assert eval_loss(m, g) == before
    assert all(torch.equal(bits(ema.state_dict()["shadow"][n]), bits(avg[n])) for n in names)
    assert loss_in != before

    # the same averaged values written with p.copy_(): the forward re-casts, and computes the same bits
    with torch.no_grad():
        for n, p in zip(names, tracked(m)):
            p.copy_(avg[n])
    assert not m._trainable_current()
    assert eval_loss(m, g) == loss_in
    assert torch.equal(greedy(m, g), toks_in)
    with torch.no_grad():
        for p, r in zip(tracked(m), raw):
            p.copy_(r)
    assert eval_loss(m, g) == before

    for _ in range(2):  # training goes on, on the fused paths
        step_update_check(m, g, opt, ema, str(dtype))
    assert ema.num_updates == 6 and opt._fallback is None and m._trainable_current()


def test_update_after_a_step_in_backward_is_ordered_behind_it():
    from klab_multimodalmodel_amd.optim import FusedAdamW, WeightEMA
    m, g = build("tiny_a")
    opt = FusedAdamW(two_groups(m), lr=3e-3, step_in_backward=True)
    ema = WeightEMA(m, decay=0.99)
    for _ in range(4):
        step_update_check(m, g, opt, ema, "step_in_backward")
    assert opt.in_backward_updates == 3 and opt._fallback is None
    # an in-backward update nobody has joined yet: update() and swap() order themselves behind it
    run(m, g).backward()
    assert m._pending_opt_stream is not None
    ema.update()
    assert m._pending_opt_stream is None
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()


def test_a_rebind_between_updates_keeps_the_flat_state():
    from klab_multimodalmodel_amd.optim import FusedAdamW, WeightEMA
    m, g = build("tiny_a")
    opt = FusedAdamW(two_groups(m), lr=3e-3)
    ema = WeightEMA(m, decay=0.9)
    step_update_check(m, g, opt, ema, "rebind")
    flat = ema._flat
    step_update_check(m, g, opt, ema, "rebind", rows=2, lt=5)  # another (B, Lt): a re-bind
    step_update_check(m, g, opt, ema, "rebind")                # and back
    assert ema._flat is flat and ema._fb_reason is None and ema.num_updates == 3
    raw = [p.detach().clone() for p in tracked(m)]
    with ema.average_parameters():
        assert m._trainable_current()
        with torch.no_grad():
            float(run(m, g, rows=2, lt=5))  # a re-bind inside the context
    assert ema._flat is flat and ema._fb_reason is None
    assert all(torch.equal(bits(p.detach()), bits(r)) for p, r in zip(tracked(m), raw))


def test_an_ema_built_before_the_first_forward_starts_from_the_construction_weights():
    from klab_multimodalmodel_amd.optim import FusedAdamW, WeightEMA
    m, g = build("tiny_a")
    ema = WeightEMA(m, decay=0.999)
    opt = FusedAdamW(two_groups(m), lr=3e-3)
    p0 = [p.detach().clone() for p in tracked(m)]
    assert ema._flat is None
    train(m, g, opt, 1)
    ema.update()
    assert ema._fb_reason is None and ema._flat is not None and ema.num_updates == 1
    e0, mask = flat_of(m, p0)
    p1, _mask = flat_of(m, tracked(m))
    w = E.weight_at(0.999, True, 1)
    assert w == E.f32(1.0 - 2.0 / 11.0)
    r = E.worst(ema._flat.cpu()[mask], p1[mask], e0[mask], w)
    print(f"WeightEMA built before the first forward: err / bound {r:.3f}")
    assert r <= 1.0
    assert not torch.equal(p1[mask], e0[mask])


@pytest.mark.parametrize("bound_first", [False, True])
def test_checkpoint_round_trip(tmp_path, bound_first):
    from klab_multimodalmodel_amd.checkpoint import AsyncCheckpointer, load_checkpoint
    from klab_multimodalmodel_amd.optim import FusedAdamW, WeightEMA
    m, g = build("tiny_a")
    opt = FusedAdamW(two_groups(m), lr=3e-3)
    ema = WeightEMA(m, decay=0.9)
    for _ in range(2):
        step_update_check(m, g, opt, ema, "checkpoint")
    ck = AsyncCheckpointer(str(tmp_path))
    path = ck.save(m, opt, None, step=2, name="e.pth", ema=ema)
    ck.wait()
    saved = ema.state_dict()
    assert set(torch.load(path, weights_only=False)["ema"]) == {"decay", "warmup", "num_updates", "shadow"}

    m2, _g = build("tiny_a")
    fresh = WeightEMA(m2, decay=0.5, warmup=False)
    if bound_first:
        with torch.no_grad():
            run(m2, g)
    assert load_checkpoint(path, m2, ema=fresh) == 2
    assert (fresh._flat is not None) == bound_first
    assert (fresh.decay, fresh.warmup, fresh.num_updates) == (0.9, True, 2)
    got = fresh.state_dict()["shadow"]
    assert set(got) == set(saved["shadow"]) == set(m2.transformer.state_dict())
    assert all(torch.equal(bits(got[k].cpu()), bits(saved["shadow"][k].cpu())) for k in got)
    # the next update, on the fused path
    opt2 = FusedAdamW(two_groups(m2), lr=3e-3)
    step_update_check(m2, g, opt2, fresh, f"resumed (bound first: {bound_first})")
    assert fresh.num_updates == 3
    m2.transformer.load_state_dict(saved["shadow"])
    # without the argument nothing changes: no "ema" key, and asking for one that is not there says so
    plain = ck.save(m, opt, None, step=2, name="plain.pth")
    ck.wait()
    assert "ema" not in torch.load(plain, weights_only=False)
    with pytest.raises(RuntimeError, match="holds no weight EMA"):
        load_checkpoint(plain, m2, ema=fresh)
    assert os.path.exists(path)


def test_a_foreign_module_on_the_gpu_takes_the_torch_path():
    from klab_multimodalmodel_amd.optim import WeightEMA
    torch.manual_seed(3)
    lin = torch.nn.Linear(33, 17).cuda()
    ema = WeightEMA(lin, decay=0.5)
    e0 = [p.detach().cpu().clone() for p in lin.parameters()]
    hist = []
    for _ in range(12):
        with torch.no_grad():
            for p in lin.parameters():
                p.add_(0.05 * torch.randn_like(p))
        ema.update()
        hist.append([p.detach().cpu().clone() for p in lin.parameters()])
    assert ema._fb_reason == "parameters not owned by one klab MyModel" and ema._flat is None and ema.num_updates == 12
    sd = ema.state_dict()["shadow"]
    for k, name in enumerate(("weight", "bias")):
        assert sd[name].is_cuda
        ref, acc = E.recurrence([h[k] for h in hist], e0[k], 0.5, True)
        assert float(((sd[name].cpu().double() - ref).abs() / acc).max()) <= 1.0
    raw = [p.detach().clone() for p in lin.parameters()]
    with ema.average_parameters():
        assert torch.equal(bits(lin.weight.detach()), bits(sd["weight"]))
    assert all(torch.equal(bits(p.detach()), bits(r)) for p, r in zip(lin.parameters(), raw))
