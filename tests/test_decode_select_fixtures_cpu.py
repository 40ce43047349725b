"""What tests/test_beam_exact_gpu.py, tests/test_logits_proc_exact_gpu.py and tests/test_sample_exact_gpu.py take for granted about
tests/beam_ref.py, tests/logits_proc_ref.py and tests/sample_ref.py, proved on the CPU:

  1. every fixture value survives its dtype, the grid sums of the top-k fixtures are exact in f32, and the log-softmax fixtures have
     their 0.25 gaps (or exact ties, by construction);
  2. the parametrisations reach what they claim: every list length of the row kernel with 2k < KMAX and 2k == KMAX, both load loops
     per dtype (and the one-thread placements really lie inside one thread), bitmap words other than 0, the partial last word, ids
     outside the vocabulary, a bad-word list longer than the workgroup, several matching n-gram windows at the history limit, a
     search that laps the 64-position sequence loop and searches that end at different steps;
  3. on the sampling fixture HF's rule and the kernel's agree on every plain setting, nothing is a boundary case except the arg-max
     at top_p = 0, and every drawn u lies at least 1e-4 from a CDF step edge (u = 0 and u = 1 - 2^-24 by their own conditions);
  4. each mutation of a reference -- the wrong answer of a subtly wrong kernel -- is rejected by the exact comparison the GPU test
     makes, on at least one fixture."""
import pytest
import torch

from tests import beam_ref as R
from tests import logits_proc_ref as P
from tests import sample_ref as S
from tests.exact_ref import bf16_exact


def _f32_exact(x):
    fin = x[~torch.isinf(x)].double()
    return bool((fin.float().double() == fin).all())


# ---- 1. exactness -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.KS)
def test_score_fixtures_are_on_the_grid(k):
    for V in R.vocabs(k):
        assert V >= 2 * k
        for lay in R.LAYOUTS:
            for kind in R.SCORE_KINDS:
                x, rs = R.scores_fixture(kind, k, V, lay)
                fin = x[~torch.isinf(x)].double()
                what = (k, V, lay, kind)
                assert x.shape == (R.B * k, V) and not torch.isnan(x).any() and not (x == float("inf")).any(), what
                assert bool(((fin * 16).round() == fin * 16).all()) and bool(((fin <= 0) & (fin >= -16)).all()), what
                first = kind in ("a1", "e1", "f1")
                if first:
                    assert torch.equal(rs, R.first_step_scores(k)), what
                    # -1e9 swallows every grid value: all finite candidates of such a beam tie
                    assert bool(((fin.float() + torch.tensor(R.NEG)) == R.NEG).all()), what
                else:
                    r64 = rs.double()
                    assert bool(((r64 * 16).round() == r64 * 16).all()) and bool(((r64 <= 0) & (r64 >= -2)).all()), what
                    # |sum| < 32 in units of 2^-4: far below 2^24 units, the f32 add is exact
                    s64 = x.double() + r64.view(-1, 1)
                    assert torch.equal((x + rs.view(-1, 1)).double(), s64), what
                if kind in ("e", "e1"):
                    assert int((~torch.isinf(x)).sum(-1).max()) < 2 * k, what
                if kind in ("f", "f1"):
                    assert int(torch.isinf(x).all(-1).view(R.B, k).sum(-1).min()) >= 1, what


@pytest.mark.parametrize("k", R.KS)
def test_logit_fixtures_have_their_gaps(k):
    for dn in ("f32", "bf16"):
        for V in R.vocabs(k):
            for lay in R.LAYOUTS:
                for row_div in sorted({1, k}):
                    for kind, tie_rows in [(kd, False) for kd in R.LOGIT_KINDS] + ([("b", True)] if row_div > 1 else []):
                        x, rs = R.logits_fixture(kind, k, V, row_div, dn, lay, tie_rows)
                        what = (k, dn, V, lay, row_div, kind, tie_rows)
                        assert bf16_exact(x) and float(x.abs().max()) <= 24.0, what
                        # the 2k + 1 best final scores of every sample (a 2k+1-st exists when k V > 2k): equal bit for bit or
                        # at least 0.25 (less f32 rounding of scores up to 128: 1e-4) apart
                        fin = (torch.log_softmax(x, -1).float().repeat_interleave(row_div, 0) + rs.view(-1, 1)).view(R.B, k * V)
                        top = torch.sort(fin, -1, descending=True)[0][:, :2 * k + 1]
                        d = top[:, :-1] - top[:, 1:]
                        assert bool(((d == 0) | (d >= 0.25 - 1e-4)).all()), (what, d)
                        assert bool((d[:, 0] == 0).all()), what  # the deliberate tie leads
                        if k * V > 2 * k:
                            assert bool((d[:, -1] >= 0.25 - 1e-4).all()), what  # the winners stand clear of the rest
                        if tie_rows and k >= 2:
                            assert bool((d[:, :3] == 0).all()), what  # two beams x two equal logits


# ---- 2. coverage --------------------------------------------------------------------------------------------------------------------
def test_topk_parametrisation_reaches_every_instantiation_and_load_loop():
    seen = {(R.kmax(k), 2 * k == R.kmax(k)) for k in R.KS}
    assert {n for n, _ in seen} == {2, 4, 8, 16, 32} and {full for _, full in seen} == {False, True}
    assert {(16, False), (16, True), (32, False), (32, True)} <= seen  # the staged 32-entry lists both ways
    assert {R.threads(k) for k in R.KS} == {128, 256}
    for esize in (4, 2):
        paths = set()
        for k in R.KS:
            for V in R.vocabs(k):
                for lay in R.LAYOUTS:
                    ld, off = R.layout(lay, V)
                    for row_div in (1, k):
                        paths |= {(R.load_path(esize, V, ld, off, r // row_div), lay) for r in range(R.B * k)}
        assert {p for p, _ in paths} == {"vector", "scalar"}, esize
        assert ("scalar", "dense") in paths and ("scalar", "odd") in paths, esize  # odd V; a row start off 16 bytes
    assert R.load_path(2, 4100, 4100, 0, 0) == "scalar" and R.load_path(4, 4100, 4100, 0, 0) == "vector"
    assert -(-4104 // (256 * 8)) == 3 and 4104 % (256 * 8) != 0  # three vector laps for bf16 at 256 threads, the last one partial
    # the one-thread placements: all 2k winners of a sample among the tokens one thread streams, on each load loop
    inside = set()
    for k in R.KS:
        for V in (1001, 4100, 4104):
            for lay in R.LAYOUTS:
                ld, off = R.layout(lay, V)
                x, _ = R.scores_fixture("b2", k, V, lay)
                for b in range(R.B):
                    r = b * k + (b + 1) % k
                    path = R.load_path(4, V, ld, off, r)
                    own = R.owned_tokens((5 + b) % R.threads(k), V, R.threads(k), 4 if path == "vector" else 0)
                    win = torch.nonzero(x[r] > -8).flatten().tolist()
                    assert len(win) == 2 * k
                    if set(win) <= set(own):
                        inside.add((R.kmax(k), path))
    assert inside >= {(n, p) for n in (2, 4, 8, 16) for p in ("vector", "scalar")} | {(32, "vector"), (32, "scalar")}, inside


def test_processor_fixtures_reach_the_bitmaps_edges():
    for V in P.PROC_VOCABS:
        F = P.forced_tokens(V)
        assert all(0 <= t < V for t in F) and F[0] == 0 and F[3] == V - 1
        if V > 32:
            assert 31 in F and 32 in F and F[4] // 32 == (V - 1) // 32
        lo, hi = P.tie_tokens(V)
        assert lo != hi and lo // 32 != hi // 32 or V <= 32
        for row_div in (1, 3):
            for cur in P.PROC_CUR:
                x, hist = P.proc_fixture(V, row_div, cur)
                assert bf16_exact(x) and hist.shape == (P.PROC_ROWS * row_div, cur)
                assert float(x.max()) == 9.0 and int((x[0] == 9.0).sum()) == 2
                if cur >= 3:
                    assert int((hist >= V).sum()) >= 1 and int((hist < 0).sum()) >= 1
                if cur >= 64:
                    inside = hist[(hist >= 0) & (hist < V)]
                    assert set(F) <= set(inside.tolist())
                    if V > 64:
                        assert len({int(t) // 32 for t in inside}) >= min(20, V // 32)  # many bitmap words, not word 0 alone
                    assert any(len(set(h)) < len(h) for h in hist.tolist())  # repeated tokens
                if cur == 1024:
                    last = hist[-1].tolist()
                    follow = {last[w + 1] for w in range(cur - 1) if last[w] == last[-1]}
                    assert len(follow) >= 2  # n-gram size 2: several windows match, banning different tokens
        st = P.proc_settings(V)
        assert max(len(kw.get("bad_words_ids", ())) for kw in st) == 1100 > 1024
        assert all([P.EOS] not in kw.get("bad_words_ids", ()) for kw in st)
    assert any(V % 32 for V in P.PROC_VOCABS) and any(V % 32 == 0 for V in P.PROC_VOCABS)


def test_scripted_searches_cover_the_sequence_loop_and_end_at_different_steps():
    ends = {}
    for k, V, Lm in R.SEARCHES:
        fn = R.scripted_scores(k, V, Lm)
        for c in range(1, Lm):
            x = fn(c)
            fin = x[~torch.isinf(x)].double()
            assert bool(((fin * 16).round() == fin * 16).all()) and float(fin.min()) >= -16 and int(torch.isinf(x).sum()) >= 1
        for es in R.SEARCH_ES:
            for lp in R.SEARCH_LP:
                st = R.search_reference(fn, R.B, k, V, Lm, dict(k=k, V=V, Lm=Lm, eos=R.EOS, lp=lp, es=es))
                ends.setdefault((k, V, Lm), set()).add(st[-1]["c"])
                # running scores: sums of at most Lm grid values >= -16: exact in f32
                rs = st[-1]["run_score"].double()
                live = rs > -1e8
                assert bool(((rs[live] * 16).round() == rs[live] * 16).all())
                if st[-1]["fin_flag"].any():
                    lens = st[-1]["fin_len"][st[-1]["fin_flag"]]
                    ends.setdefault(("lens", k), set()).update(lens.tolist())
    assert max(ends[(4, 50, 70)]) >= 66  # positions past 64: the second lap of the kernel's sequence loop
    assert all(len(ends[s]) >= 2 for s in R.SEARCHES)
    assert all(len(ends[("lens", k)]) >= 3 for k, _, _ in R.SEARCHES)


# ---- 3. the sampling fixture ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", ["f32", "bf16"])
@pytest.mark.parametrize("V", S.SAMPLE_VOCABS)
def test_sampling_fixture_has_no_boundary_cases(V, dn):
    x = S.sample_fixture(V, dn)
    fin = x[~torch.isinf(x)]
    assert bf16_exact(fin) if dn == "bf16" else _f32_exact(fin)
    groups, m = S.level_count(V)
    assert int((x[:4] > -10).sum(-1).min()) == m == int((x[:4] > -10).sum(-1).max()) and float(x[x <= -10].max()) == -40.0
    bg = x[0][x[0] <= -10]
    if not (dn == "bf16" and V > 15000):
        assert len(set(bg.tolist())) == len(bg)  # pairwise distinct
    assert int(torch.isinf(x[4:]).sum(-1).min()) == min(5, V - m - 2 if V - m > 2 else 0) or V == 5
    settings = S.sample_settings(V, dn, S.TEMPERATURES if V < 32768 else (1.0,))
    plain = flagged = high = low = 0
    for t, k, p, is_plain in settings:
        x32 = x.float()
        kept = S.kept_reference(x32, t, k, p)
        assert bool(kept.any(-1).all())
        if is_plain:
            plain += 1
            assert torch.equal(kept, ~torch.isinf(S.hf_warp(x32, t, k, p))), (V, dn, t, k, p)
            flags = S.boundary_tokens(x32[:4], t, k, p)
            if flags.any():
                flagged += 1
                assert p == 0.0 and torch.equal(flags, x32[:4] == x32[:4].max(-1, keepdim=True)[0]), (V, dn, t, k, p)
        # the draws: every u (as the f32 the kernel gets) at least 1e-4 inside its token's CDF step, u = 0 and u = 1 - 2^-24 excepted
        s = S.scaled(x32, t).double().masked_fill(~kept, -float("inf"))
        cdf = torch.softmax(s, -1).cumsum(-1)
        cdf = cdf / cdf[:, -1:]
        for r, u, tok in S.draw_points(x32, t, kept):
            assert bool(kept[r, tok])
            u32 = float(torch.tensor(u, dtype=torch.float32))
            before = float(cdf[r, tok - 1]) if tok else 0.0
            if u == 0.0:
                low += 1
                assert tok == int(torch.nonzero(kept[r])[0])
            elif u == S.U_HIGH:
                high += 1
                assert u32 == u and before < u - 1e-5 and float(cdf[r, tok]) > u
            else:
                assert before + 1e-4 <= u32 <= float(cdf[r, tok]) - 1e-4, (V, dn, t, k, p, r, u)
    if V < 32768:
        assert plain == (69 if V == 5 else 117) and flagged == 18, (plain, flagged)
    assert len(settings) > plain and low == 8 * len(settings) and high >= 6 * len(settings), (len(settings), plain, low, high)


# ---- 4. mutations -------------------------------------------------------------------------------------------------------------------
TOPK_MUTATIONS = ("row tie high", "merge tie high", "list truncated", "last token dropped", "token V read", "beam = r / k",
                  "sentinel leak", "row ranked before the add")


@pytest.mark.parametrize("mut", TOPK_MUTATIONS)
def test_topk_mutations_are_rejected(mut):
    rejected = []
    for k in (1, 3, 9):
        for V in (2 * k, 37, 1001):
            ld, off = R.layout("odd", V)
            for kind in R.SCORE_KINDS:
                x, rs = R.scores_fixture(kind, k, V, "odd")
                _, view = R.device_layout(x, ld, off, float("inf"))  # what the kernel is handed: +inf past V
                want = R.topk_reference(view, rs, k, V, 1, True)
                got = R.topk_reference(view, rs, k, V, 1, True, mut=mut)
                if not (torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])):
                    rejected.append((k, V, kind))
    assert rejected, mut
    if mut == "row ranked before the add":  # only the first-step scores round distinct sums to one value
        assert {kind for _, _, kind in rejected} <= {"e1", "f1"}
    if mut == "sentinel leak":
        assert {kind for _, _, kind in rejected} <= {"e", "e1", "f", "f1"}


def test_topk_row_div_mutation_is_rejected():
    for k in (3, 9):
        x, rs = R.logits_fixture("b", k, 37, k, "f32")
        want = R.topk_reference(x.float(), rs, k, 37, k, False)
        got = R.topk_reference(x.float(), rs, k, 37, k, False, mut="row_div ignored")
        assert not torch.equal(got[1], want[1]), k  # indices are compared exactly


UPDATE_MUTATIONS = ("pool tie to candidate", "fin_len kept")


@pytest.mark.parametrize("mut", UPDATE_MUTATIONS)
def test_update_mutations_are_rejected(mut):
    g = torch.Generator().manual_seed(3)
    rejected = []
    for k in (2, 3, 8):
        for lp in (0.0, 1.0):
            for c in (2, 5):
                cfg = dict(k=k, V=R.UPDATE_V, Lm=8, eos=R.EOS, lp=lp, es=0)
                st, cs, ci = R.tie_scenario(k, 8, c, lp, g)
                want = R.update_reference(st, cs, ci, c, cfg)
                # the ties are there and are resolved pool entry first, then the lower candidate
                assert bool((want["fin_score"][:, 0] == want["fin_score"][:, 1]).all()) and bool((want["fin_len"][:, 0] == c - 1).all())
                assert bool((want["fin_len"][:, 1] == c).all()) and bool((want["run_score"][:, 0] == want["run_score"][:, 1]).all())
                assert torch.equal(want["tok"][:, :2], (ci % R.UPDATE_V)[:, 2:4])
                bad = R.state_mismatches(R.update_reference(st, cs, ci, c, cfg, mut=mut), want, c, slot=False)
                if bad:
                    rejected.append((k, lp, c, bad))
    assert rejected, mut


@pytest.mark.parametrize("mut", ["no swap at step 3", "slot copied short", "fin_len kept"])
def test_search_mutations_are_rejected(mut):
    rejected = []
    for k, V, Lm in R.SEARCHES[1:]:
        fn = R.scripted_scores(k, V, Lm)
        cfg = dict(k=k, V=V, Lm=Lm, eos=R.EOS, lp=1.0, es=0)
        want = R.search_reference(fn, R.B, k, V, Lm, cfg)
        got = R.search_reference(fn, R.B, k, V, Lm, cfg, mut=mut)
        for a, b in zip(got[1:], want[1:]):
            bad = R.state_mismatches(a, b, b["c"])
            if bad:
                rejected.append((k, b["c"], bad))
                break
    assert rejected, mut
    if mut == "slot copied short":
        assert all(bad == ["slot"] for _, _, bad in rejected)


PROC_MUTATIONS = ("bit off by one", "penalty twice", "id wrapped modulo V", "last window skipped")


@pytest.mark.parametrize("mut", PROC_MUTATIONS)
def test_processor_mutations_are_rejected(mut):
    rejected = []
    for V in (33, 1057):
        for cur in (3, 64):
            x, hist = P.proc_fixture(V, 1, cur)
            for si, kw in enumerate(P.proc_settings(V)):
                want = P.process_reference(hist, x.float(), V, **kw)
                if not torch.equal(P.process_reference(hist, x.float(), V, mut=mut, **kw), want):
                    rejected.append((V, cur, si))
    assert rejected, mut


def test_processor_reference_agrees_with_the_restatement_of_hf():
    """on in-range histories the kernel's statement and the restatement of HF's processors are the same function"""
    for V in (33, 1057):
        x, hist = P.proc_fixture(V, 1, 64)
        hist = hist.clamp(0, V - 1)
        for kw in P.proc_settings(V):
            for log_softmax in (False, True):
                got = P.process_reference(hist, x.float(), V, log_softmax=log_softmax, **kw)
                want = P.hf_process(hist, x.float(), log_softmax=log_softmax, **kw)
                assert torch.equal(torch.isinf(got), torch.isinf(want))
                fin = ~torch.isinf(want)
                assert torch.allclose(got[fin], want[fin], rtol=1e-6, atol=2e-6 if log_softmax else 0)


@pytest.mark.parametrize("mut", ["kept rule with <=", "tie group split at the k-th value"])
def test_sampling_kept_mutations_are_rejected(mut):
    rejected = []
    for V in (5, 33):
        x = S.sample_fixture(V, "bf16").float()
        for t, k, p, plain in S.sample_settings(V, "bf16"):
            if not torch.equal(S.kept_reference(x, t, k, p, mut=mut), S.kept_reference(x, t, k, p)):
                rejected.append((V, t, k, p))
                assert not plain  # on the plain settings no tie group meets a boundary
    assert rejected, mut


def test_sampling_draw_mutation_is_rejected():
    x = S.sample_fixture(33, "f32").float()
    kept = S.kept_reference(x, 1.0, 0, 1.0)
    want = {(r, round(u, 9)): tok for r, u, tok in S.draw_points(x, 1.0, kept)}
    got = {(r, round(u, 9)): tok for r, u, tok in S.draw_points(x, 1.0, kept, mut="descending ids")}
    # the descending draw's midpoints are other u's: feed its u's to the ascending CDF and the tokens differ
    s = S.scaled(x, 1.0).double()
    cdf = torch.softmax(s, -1).cumsum(-1)
    wrong = sum(1 for (r, u), tok in got.items() if u and int((cdf[r] / cdf[r, -1] > u).long().argmax()) != tok)
    assert wrong >= 8 and want
