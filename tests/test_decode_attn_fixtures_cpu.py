"""What tests/test_decode_attn_exact_gpu.py takes for granted about tests/decode_attn_ref.py, proved on the CPU:

  1. every operand and every expected value of the exact fixture survives a round trip through its dtype (exact_ref.bf16_exact for
     bf16), every score is 0 or <= -200, every (row, head) has 1, 2 or 4 chosen keys, and every sum the kernel can form on the way is a
     sum of integers (in units of the column's power of two) whose absolute values stay below 2^24: exact in f32 in any order;
  2. the chosen keys cover what the kernel's lane split makes special (listed in the test);
  3. the device layouts hold the logical operands where the kernel's address arithmetic reads, NaN everywhere else, and no slot
     number outside the cache;
  4. each mutation of the reference (last key dropped; key Lk also read; one slot entry replaced by another valid slot; the kv_group
     division off by one row; head h reading head h + 1's bias row; the rescale of a lane's later laps left out) is rejected by the
     exact assertion and by the per-element bound, on every (row, head) it touches."""
import pytest
import torch

from tests import decode_attn_ref as D
from tests.exact_ref import bf16_exact

DTYPES = ("f32", "bf16")


def _fits(x, dtype):
    return bf16_exact(x) if dtype == torch.bfloat16 else bool((x.float().double() == x).all())


@pytest.mark.parametrize("dn", DTYPES)
def test_exact_fixture_is_exact_and_order_independent(dn):
    dtype = D.DT[dn]
    for form, g, Lk, dk, wb in D.cases():
        f = D.exact_fixture(dn, form, g, Lk, dk, wb)
        what = (dn, form, g, Lk, dk, wb)
        for t in (f.q, f.K, f.V, f.want):
            assert _fits(t, dtype), what
        assert f.bias is None or _fits(f.bias, torch.float32)
        r = D.reference(f.q, f.K, f.V, f.bias, Lk, f.kv_slot, g)
        S = r["S"]
        assert bool(((S == 0) | (S <= -200)).all()), what
        for rr in range(f.rows):
            for h in range(D.H):
                ch = f.chosen[rr][h]
                assert len(ch) in (1, 2, 4) and len(set(ch)) == len(ch) and max(ch) < Lk, what
                if Lk > 1:
                    assert (S[rr, h] == 0).nonzero().flatten().tolist() == sorted(ch), (what, rr, h)
        assert torch.equal(r["ctx"], f.want), what
        assert torch.equal(D.lanes_reference(S, r["V"]), f.want), what  # the kernel's own order gives the same number
        units = (r["V"] / f.scale[None, None]).abs()  # [R, Lk, H, dk]: integers
        assert bool((units == units.round()).all()) and float(units.sum(1).max()) < 2.0 ** 24, what
        # the chosen values alone: a sum below 2^8 (bf16) / 2^15 (f32) units, so the mean keeps every bit
        assert float((f.want / f.scale[None]).abs().max()) < (2.0 ** 6 if dtype == torch.bfloat16 else 2.0 ** 13), what


def test_chosen_keys_cover_the_lane_split():
    seen = set()
    for Lk in D.LKS:
        pats = D.patterns(Lk)
        assert 1 <= len(pats) <= 8 and len(pats) <= D.R * D.H  # one-hot columns inside dk = 8; every pattern used by some (row, head)
        for p in pats:
            assert len(p) in (1, 2, 4) and all(0 <= j < Lk for j in p)
            if 0 in p:
                seen.add("key 0")
            if Lk - 1 in p and Lk > 1:
                seen.add("key Lk-1")
            if 63 in p and 64 in p:
                seen.add("63 and 64")
            if any(j + 64 in p for j in p):
                seen.add("one lane, two laps")
            for j in p:
                earlier = [i for i in range(j % 64, j, 64)]
                if j >= 64 and earlier and not any(i in p for i in earlier):
                    seen.add(f"lap {j // 64 + 1} behind unchosen keys")
                if j < 64 and j + 64 < Lk and j + 64 not in p:
                    seen.add("lap 1 with unchosen keys behind it")
        if Lk < 64:
            seen.add("lanes without a key")
        if Lk > 1:
            mk = D.masked_keys(Lk, D.H)
            assert mk is not None and all(mk[h] != mk[h + 1] for h in range(D.H - 1)) and not any(m in p for m in mk for p in pats)
    assert seen >= {"key 0", "key Lk-1", "63 and 64", "one lane, two laps", "lap 2 behind unchosen keys", "lap 3 behind unchosen keys",
                    "lap 1 with unchosen keys behind it", "lanes without a key"}, seen


@pytest.mark.parametrize("dn", DTYPES)
def test_layouts_hold_the_operands_and_nan_elsewhere(dn):
    dtype = D.DT[dn]
    for form, g, Lk, dk, wb in D.cases():
        for c in (D.exact_fixture(dn, form, g, Lk, dk, wb), D.random_case(dn, form, g, Lk, dk, wb)):
            q, k, v, kw, whole = D.layout(c, dtype)
            r = D.reference(c.q, c.K, c.V, c.bias, Lk, c.kv_slot, g)
            qq, kk, vv, bb = D.read_like_the_kernel(q, k, v, kw)
            srow = D.key_rows(c.rows, Lk, c.kv_slot, g)
            j = torch.arange(Lk)[None].expand(c.rows, Lk)
            assert torch.equal(qq, c.q) and torch.equal(kk, c.K[srow, j]) and torch.equal(vv, r["V"]), (dn, form, g, Lk, dk, wb)
            S, inner = c.K.shape[0], D.H * dk
            finite = {n: None if t is None else int((~torch.isnan(t.float())).sum()) for n, t in whole.items()}
            if form == "slot":  # the cache holds k | v of Lk rows per slot and the one q block of every row
                assert kw["slot_ld"] >= Lk and int(kw["kv_slot"].min()) >= 0 and int(kw["kv_slot"].max()) < S
                assert finite["kv"] == S * Lk * 2 * inner + c.rows * inner and whole["q"] is None
            else:
                assert finite["kv"] == S * Lk * 2 * inner and finite["q"] == c.rows * inner
            if wb:
                assert torch.equal(bb, c.bias[:, :Lk].float().double()) and finite["bias"] == D.H * Lk
            else:
                assert kw["bias_row"] is None and whole["bias"] is None


def _mutants(c, r, Lk, g, with_bias, exact):
    """(mutation, mutated fp64 result, bool [R, H] of the (row, head) pairs it touches)"""
    nrows = c.rows
    every = torch.ones(nrows, D.H, dtype=torch.bool)
    out = []
    if Lk > 1:
        hit = torch.tensor([[Lk - 1 in c.chosen[rr][h] for h in range(D.H)] for rr in range(nrows)]) if exact else every
        out.append(("drop_last", D.mutated("drop_last", c.q, c.K, c.V, c.bias, Lk, c.kv_slot, g), hit))
    out.append(("read_extra", D.mutated("read_extra", c.q, c.K, c.V, c.bias, Lk, c.kv_slot, g), every))
    for h in range(D.H if exact else 1):
        key = torch.tensor([min(c.chosen[rr][h]) for rr in range(nrows)]) if exact else torch.full((nrows,), Lk - 1)
        hit = every.clone()
        if exact:
            hit[:] = False
            hit[:, h] = True
        out.append(("slot_swap", D.mutated("slot_swap", c.q, c.K, c.V, c.bias, Lk, c.kv_slot, g, key), hit))
    if c.form == "group":
        S = c.K.shape[0]
        moved = ((torch.arange(nrows) + 1) // g) % S != torch.arange(nrows) // g
        out.append(("group_off", D.mutated("group_off", c.q, c.K, c.V, c.bias, Lk, c.kv_slot, g), moved[:, None] & every))
    if with_bias and Lk > 1:
        hit = every.clone()
        hit[:, D.H - 1] = False
        out.append(("bias_next_head", D.mutated("bias_next_head", c.q, c.K, c.V, c.bias, Lk, c.kv_slot, g), hit))
    if Lk > 64:
        if exact:
            hit = torch.tensor([[any(j >= 64 and not all(i in c.chosen[rr][h] for i in range(j % 64, j, 64)) for j in c.chosen[rr][h])
                                 for h in range(D.H)] for rr in range(nrows)])
        else:
            hit = r["S"][:, :, 64] > r["S"][:, :, 0]  # lane 0's maximum rises on its second lap, at a planted key
        out.append(("no_rescale", D.mutated("no_rescale", c.q, c.K, c.V, c.bias, Lk, c.kv_slot, g), hit))
    return out


@pytest.mark.parametrize("dn", DTYPES)
def test_mutations_are_rejected_by_the_exact_fixture(dn):
    dtype = D.DT[dn]
    count = {m: 0 for m in D.MUTATIONS}
    for form, g, Lk, dk, wb in D.cases():
        f = D.exact_fixture(dn, form, g, Lk, dk, wb)
        r = D.reference(f.q, f.K, f.V, f.bias, Lk, f.kv_slot, g)
        for mut, got, hit in _mutants(f, r, Lk, g, wb, True):
            wrong = (got.to(dtype).double() != f.want).any(-1)
            assert bool(wrong[hit].all()), (dn, form, g, Lk, dk, wb, mut, (hit & ~wrong).nonzero().tolist())
            count[mut] += int(hit.sum())
    assert all(n > 0 for n in count.values()), count


@pytest.mark.parametrize("dn", DTYPES)
def test_mutations_are_rejected_by_the_bound(dn):
    dtype = D.DT[dn]
    count = {m: 0 for m in D.MUTATIONS}
    lane0, pairs = 0, 0
    for form, g, Lk, dk, wb in D.cases(random_only=True):
        c = D.random_case(dn, form, g, Lk, dk, wb)
        r = D.reference(c.q, c.K, c.V, c.bias, Lk, c.kv_slot, g)
        bnd = D.bound(r, Lk, dk, dtype)
        own = r["ctx"].to(dtype).double() if dtype == torch.bfloat16 else r["ctx"]
        assert not bool(D.rejected(own, r["ctx"], bnd).any())  # the bound admits the reference itself (rounded for bf16)
        assert not bool(D.rejected(D.lanes_reference(r["S"], r["V"]).to(dtype).double(), r["ctx"], bnd).any())  # ... and the kernel's order
        for mut, got, hit in _mutants(c, r, Lk, g, wb, False):
            rej = D.rejected(got.to(dtype).double(), r["ctx"], bnd)
            assert bool(rej[hit].all()), (dn, form, g, Lk, dk, wb, mut, (hit & ~rej).nonzero().tolist())
            count[mut] += int(hit.sum())
            if mut == "no_rescale":
                lane0, pairs = lane0 + int(hit.sum()), pairs + hit.numel()
    assert all(n > 0 for n in count.values()), count
    assert 10 * lane0 >= 9 * pairs, (lane0, pairs)  # the planted key 64 makes nearly every (row, head) a witness of the rescale
