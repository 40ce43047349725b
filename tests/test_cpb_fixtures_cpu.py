"""What tests/test_cpb_exact_gpu.py takes for granted about tests/cpb_ref.py, proved on the CPU:

  1. the exact forward fixture is representable in f32, has pre-activations that are exactly 0 and negative ones, and every table entry is
     a sum whose terms' absolute values stay below 2^24 units of 1/8;
  2. the exact backward fixture: every operand is an f32 number, b (1 - b / 16) is 0, 3, 4, 3, 0, every table row used by the cases that
     say so, and for every element of dtable, dW0, db0 and dW2 the absolute values of its terms (initial content and a preset dtable
     included) add up to less than 2^24 units: the result does not depend on the order of the atomics or of the reductions;
  3. each mutation of the reference (gate >= instead of >; index read transposed; table row ntab - 1 dropped; heads >= 16 dropped from
     dW2; dW0's columns swapped; hidden units j >= 16 floor(nh / 16) dropped; dtable not cleared when dtable_zeroed = 0) is rejected by
     the exact fixtures, and by the per-element bound in at least nine of ten elements whose value it changes (a change below the
     bound is one no test of a f32 kernel can see) and in at least one element of every output it changes."""
import pytest
import torch

from tests import cpb_ref as C


def _f32(x):
    return bool((x.float().double() == x).all())


def test_forward_fixture_is_exact():
    zeros = negatives = 0
    for w in C.FWD_W:
        for H in C.FWD_H:
            for nh in C.FWD_NH:
                fx = C.fwd_exact_fixture(w, H, nh)
                r = fx.ref
                for t in (fx.coords, fx.w0, fx.b0, fx.w2, r["pre"], r["hidden"], r["table"]):
                    assert _f32(t) and bool((t * 8 == (t * 8).round()).all()), (w, H, nh)
                assert float((r["hidden"].abs() @ fx.w2.abs().T).max()) * 8 < 2.0 ** 24
                zeros += int((r["pre"] == 0).sum())
                negatives += int((r["pre"] < 0).sum())
                assert int((r["pre"] == 0).sum()) > 0 and int((r["pre"] < 0).sum()) > 0 and int((r["pre"] > 0).sum()) > 0, (w, H, nh)
                assert int(fx.index.min()) == 0 and int(fx.index.max()) == fx.ntab - 1 and fx.index.numel() == fx.n ** 2
    assert zeros > 100 and negatives > 100


def test_backward_fixture_is_exact_and_order_independent():
    for case in C.bwd_exact_cases():
        ntab, n, real, H, nh = case
        fx = C.bwd_exact_fixture(*case)
        for t in (fx.coords, fx.btab, fx.bias, fx.dbias, fx.hidden, fx.w2, fx.dbtab):
            assert _f32(t), case
        assert set(fx.btab.flatten().tolist()) <= {0.0, 4.0, 8.0, 12.0, 16.0}
        slope = fx.btab * (1.0 - fx.btab * 0.0625)
        assert set(slope.flatten().tolist()) <= {0.0, 3.0, 4.0} and _f32(1.0 - fx.btab * 0.0625)
        assert int(fx.index.min()) >= 0 and int(fx.index.max()) == ntab - 1 and fx.index.numel() == n * n
        assert 0.2 < float((fx.hidden == 0).double().mean()) < 0.5 and bool((fx.hidden >= 0).all())
        assert torch.equal(fx.bias, C.dense(fx.btab, fx.index, n))
        for dtable0 in (None, torch.full((ntab, H), 2.0, dtype=torch.float64)):
            r = C.backward(fx, dtable0=dtable0)
            assert bool((r["dtable"][ntab - 1] != 0).all()), case  # the last row carries a gradient on every head
            for k in C.OUTPUTS:
                unit = 8.0 if k == "dw0" else 1.0
                assert bool((r[k] * unit == (r[k] * unit).round()).all()) and _f32(r[k]), (case, k)
                assert float(r["abs_" + k].max()) * unit < 2.0 ** 24, (case, k, float(r["abs_" + k].max()))
            # inside the MLP backward every partial sum is bounded by the same sums: g's by abs_g
            assert float(r["parts"]["abs_g"].max()) < 2.0 ** 24
        # the table form on the scattered gradient is the same computation
        dt = fx.dbtab * slope
        assert torch.equal(dt, C.backward(fx)["dtable"])


def _changed_and_rejected(ref, mutant, bounds):
    out = {}
    for k in C.OUTPUTS:
        a, b = ref[k], mutant[k]
        changed = ((a - b).abs() > 2.0 ** -40 * ref["abs_" + k]) | torch.isnan(b)  # more than the fp64 evaluation's own noise
        rejected = ((a - b).abs() > bounds[k]) | torch.isnan(b)
        out[k] = (int(changed.sum()), int((changed & rejected).sum()))
    return out


def _applies(mut, H, nh):
    return not (mut == "heads_ge16_dropped" and H <= 16) and not (mut == "tail_units_dropped" and nh % 16 == 0)


def test_mutations_are_rejected_by_the_exact_fixtures():
    seen = {m: 0 for m in C.MUTATIONS}
    for case in C.bwd_exact_cases():
        ntab, n, real, H, nh = case
        fx = C.bwd_exact_fixture(*case)
        ref = C.backward(fx)
        for mut in C.MUTATIONS:
            if not _applies(mut, H, nh):
                continue
            m = C.backward(fx, mut)
            wrong = [k for k in C.OUTPUTS if not torch.equal(m[k], ref[k])]
            assert wrong, (case, mut)
            seen[mut] += 1
            if mut in ("gate_ge", "last_row_dropped"):
                assert "dw0" in wrong and "db0" in wrong, (case, mut, wrong)
            if mut in ("heads_ge16_dropped", "last_row_dropped", "tail_units_dropped"):
                assert "dw2" in wrong, (case, mut, wrong)
            if mut in ("index_transposed", "dtable_not_cleared"):
                assert wrong == list(C.OUTPUTS) or (mut == "index_transposed" and "dtable" in wrong), (case, mut, wrong)
    assert all(v > 0 for v in seen.values()), seen


def test_mutations_are_rejected_by_the_bound():
    seen = {m: 0 for m in C.MUTATIONS}
    for w, pw, H, nh in C.BWD_RANDOM:
        fx = C.bwd_random_fixture(w, pw, H, nh)
        ref = C.backward(fx)
        bounds = C.bwd_bounds(fx, ref)
        for k in C.OUTPUTS:  # the bound is far below the values it guards
            assert float((bounds[k] / ref["abs_" + k].clamp_min(1e-30)).max()) < 2e-4, k
        for mut in C.MUTATIONS:
            if not _applies(mut, H, nh):
                continue
            m = C.backward(fx, mut)
            res = _changed_and_rejected(ref, m, bounds)
            assert any(c for c, _ in res.values()), (w, pw, H, nh, mut)
            for k, (changed, rejected) in res.items():
                if changed:
                    assert rejected >= 1 and 10 * rejected >= 9 * changed, (w, pw, H, nh, mut, k, changed, rejected)
            seen[mut] += 1
    assert all(v > 0 for v in seen.values()), seen
