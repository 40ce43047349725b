"""What tests/test_metrics_gpu.py takes for granted, proved without a GPU: the reference of tests/metrics_ref.py on the issue's anchor
values and on cases done by hand, the fixture set's coverage, the host path of metrics.caption_stats and metrics.sentence_scores
against the reference, CaptionMetrics against the reference corpus numbers, every ValueError, and the entry point's declaration."""
import math
import os
import re

import pytest
import torch

from tests import metrics_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = M.EOS
REL = 1e-12


def close(got, want, rel=REL):
    return abs(got - want) <= rel * abs(want)


def anchor_tensors(hyps):
    """hyp [len(hyps), 9] and refs [len(hyps), 2, 8] of the anchor sentences (every image has the two anchor references)"""
    hyp = torch.tensor([M.hyp_row(M.ids(h), 9) for h in hyps])
    refs = torch.tensor([[M.ref_row(M.ids(r), 8) for r in M.ANCHOR_REFS]] * len(hyps))
    return hyp, refs


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hyp", list(M.ANCHORS))
def test_anchor_rows(hyp):
    want_stats, bleu1, bleu4, rouge = M.ANCHORS[hyp]
    row = M.stats_row(M.ids(hyp), [M.ids(r) for r in M.ANCHOR_REFS])
    assert row == want_stats + [0, 0]
    s = M.sentence(row)
    print(hyp, s)
    assert close(s[0], bleu1) and close(s[3], bleu4) and close(s[4], rouge)
    from klab_multimodalmodel_amd import metrics
    h, refs = anchor_tensors([hyp])
    got = metrics.caption_stats(h, refs)
    assert got.tolist() == [[want_stats + [0, 0]]]
    sc = metrics.sentence_scores(got)[0, 0].tolist()
    assert close(sc[0], bleu1) and close(sc[3], bleu4) and close(sc[4], rouge)


def test_a_hypothesis_equal_to_one_reference():
    for ref in M.ANCHOR_REFS:
        row = M.stats_row(M.ids(ref), [M.ids(r) for r in M.ANCHOR_REFS])
        assert row[0:4] == row[4:8] and row[8] == row[9] == row[10] == row[11] == row[12]
        assert M.sentence(row)[4] == 1.0
        from klab_multimodalmodel_amd import metrics
        got = metrics.caption_stats(*anchor_tensors([ref]))
        assert got.view(-1).tolist() == row and float(metrics.sentence_scores(got)[0, 0, 4]) == 1.0


def test_units_lcs_and_rules_by_hand():
    assert M.units([5, 6, EOS, 7]) == [5, 6] and M.units([5, 6, EOS, 7], count_eos=True) == [5, 6, EOS]
    assert M.units([5, -100, 6]) == [5] and M.units([5, 0xFFFF, 6]) == [5] and M.units([5, 0xFFFE]) == [5, 0xFFFE]
    assert M.lcs([1, 2, 3, 4, 5], [2, 4, 5, 1]) == 3 and M.lcs([], [1]) == 0 and M.lcs([7, 7, 7], [7]) == 1
    assert M.lcs(list("AGGTAB"), list("GXTXAYB")) == 4
    # no present reference: zeros.  A present reference without units counts, takes part in the closest length and is no recall pair
    assert M.stats_row([5, 6], []) == [0] * 16
    assert M.stats_row([5, 6], [[]]) == [0, 0, 0, 0, 2, 1, 0, 0, 2, 0, 0, 0, 0, 1, 0, 0]
    assert M.stats_row([5], [[], [5, 6, 7]]) == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 3, 2, 0, 0]
    assert M.stats_row([], [[5, 6]]) == [0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 2, 1, 0, 0]
    # clipping: four 5s against references with two and three of them
    assert M.stats_row([5, 5, 5, 5], [[5, 5, 9], [5, 9, 5, 5]])[0:4] == [3, 1, 0, 0]
    assert M.sentence([0] * 16) == [0.0] * 5 and M.sentence(M.stats_row([], [[5, 6]])) == [0.0] * 5


def test_the_fixture_set_holds_what_the_gpu_test_relies_on():
    cases = M.cases()
    for ce in (False, True):
        c = cases[f"lengths count_eos={ce}"]
        want = M.case_reference(f"lengths count_eos={ce}")
        assert want[:, 8].tolist() == [0, 1, 3, 4, 63, 64, 2, 5, 62] and want[:, 7].tolist() == [0, 0, 0, 1, 60, 61, 0, 2, 59]
        assert tuple(c["hyp"].shape) == (9, 65) and EOS not in c["hyp"][5].tolist()  # 64 units in 65 columns without an EOS
        assert sorted(len(M.units(r, EOS, ce)) for r in c["refs"][0].tolist()) == [3, 5, 64]
        assert bool((want[:, 13] == 3).all()) and bool((want[1:, 0] > 0).all())
        b, wb = cases[f"batch count_eos={ce}"], M.case_reference(f"batch count_eos={ce}")
        assert tuple(b["hyp"].shape) == (35, 20) and tuple(b["refs"].shape) == (7, 5, 16) and b["n_h"] == 5
        absent = (b["refs"][:, :, 0] < 0)
        assert absent[1].tolist() == [True, False, False, False, False] and absent[2].tolist() == [False, True, False, True, False]
        assert absent[3].tolist() == [True, True, True, True, False] and bool(absent[6].all()) and not bool(absent[0].any())
        assert bool((wb[30:] == 0).all())  # no present reference: rows of zeros
        assert M.units(b["refs"][4, 1].tolist(), EOS, ce) == [] and int(b["refs"][4, 1, 0]) >= 0  # present, no units
        assert bool((wb[20:25, 13] == 5).all())  # ... and it counts
        assert int(b["hyp"].max()) <= 5 or ce  # the 4-id vocabulary (0xFFFF only where count_eos needs it)
        assert bool((wb[:30:5, 8] == (1 if ce else 0)).all())  # EOS first
        assert bool((wb[1:30:5, 8] == 19).all())  # no EOS: all 19 tokens
        junk = b["hyp"][3].tolist()
        assert junk.index(EOS) < 19 and any(t > 1 for t in junk[junk.index(EOS) + 1:])  # junk behind the EOS
        assert int((wb[:30, 0:4] < wb[:30, 4:8]).sum()) > 0 and int(wb[:30, 3].max()) > 0  # clipping bites, order 4 matches
    s = cases["sixteen references"]
    assert (s["refs"][:, :, 0] < 0).tolist() == [[j in (0, 7, 15) for j in range(16)]] * 2
    assert bool((M.case_reference("sixteen references")[:, 13] == 13).all())
    one = M.case_reference("one reference")
    assert one[0, 0:4].tolist() == one[0, 4:8].tolist() and one[1].tolist() == [0] * 16 and one[2, 0:4].tolist() == [0] * 4
    assert one[2, 10:14].tolist() == [0, 0, 9, 1]
    e = cases["extreme ids"]
    assert int(e["hyp"].max()) == 65534 and sorted(set(e["hyp"][:, 1:].flatten().tolist())) == [0, 1, 2, 65534]
    assert bool((M.case_reference("extreme ids")[:, 0] > 0).all())
    t = M.case_reference("ties")
    assert t[0, 8:10].tolist() == [5, 4]  # 4 and 6 are equally close to 5: the shorter
    assert t[1, 10:13].tolist() == [3, 3, 6] and t[2, 10:13].tolist() == [3, 2, 4]  # 3 / 6 = 2 / 4: the lower index
    shapes = {(c["refs"].shape[0], c["n_h"], c["refs"].shape[1]) for c in cases.values()}
    assert {s_[0] for s_ in shapes} >= {1, 2, 3, 7} and {s_[1] for s_ in shapes} >= {1, 5, 9} and {s_[2] for s_ in shapes} >= {1, 5, 16}


# ---- the host path of the package ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.cases()))
def test_host_path_equals_the_reference(name):
    from klab_multimodalmodel_amd import metrics
    c = M.cases()[name]
    want = M.case_reference(name)
    got = metrics.caption_stats(c["hyp"], c["refs"], EOS, c["count_eos"])
    B = c["refs"].shape[0]
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, c["n_h"], 16)
    assert torch.equal(got.view(-1, 16), want), (got.view(-1, 16) != want).nonzero()[:4].tolist()
    scores = metrics.sentence_scores(got).view(-1, 5)
    assert scores.dtype == torch.float64
    for r in range(want.shape[0]):
        for k, (g, w) in enumerate(zip(scores[r].tolist(), M.sentence(want[r].tolist()))):
            assert close(g, w), (name, r, k, g, w)
        if int(want[r, 13]) == 0:
            assert scores[r].tolist() == [0.0] * 5
    assert tuple(metrics.sentence_scores(got[0, 0]).shape) == (5,)


def test_a_2d_hypothesis_tensor_is_one_caption_per_image():
    from klab_multimodalmodel_amd import metrics
    c = M.cases()["one reference"]
    assert tuple(metrics.caption_stats(c["hyp"], c["refs"]).shape) == (3, 1, 16)


def corpus_batches(ce):
    """the first hypothesis-per-image slices of two cases with the same count_eos as two batches of different B, L, R and Lr"""
    out = []
    for name, pick in ((f"batch count_eos={ce}", 3), ("sixteen references", 0)):
        c = M.cases()[name]
        out.append((c["hyp"][pick::c["n_h"]].contiguous(), c["refs"]))
    return out


@pytest.mark.parametrize("ce", [False, True])
def test_caption_metrics_over_two_batches_is_the_corpus_reference(ce):
    from klab_multimodalmodel_amd import metrics
    batches = corpus_batches(ce)
    rows = [r for hyp, refs in batches for r in M.stats(hyp, refs, 1, EOS, ce).tolist()]
    want = M.corpus(rows)
    assert want["images"] == 6 + 2 and len(rows) == 7 + 2  # the image without references is skipped
    cm = metrics.CaptionMetrics(eos_token_id=EOS, count_eos=ce)
    assert cm.compute() == dict(zip(M.NAMES, [0.0] * 5), images=0)
    for hyp, refs in batches:
        cm.update(hyp, refs)
    assert cm.sums.dtype == torch.float64 and tuple(cm.sums.shape) == (12,)
    assert cm.sums[:10].tolist() == [float(sum(r[k] for r in rows)) for k in range(10)] and float(cm.sums[11]) == 8.0
    got = cm.compute()
    print(got, want)
    assert list(got) == list(M.NAMES) + ["images"] and got["images"] == 8
    for k in M.NAMES:
        assert close(got[k], want[k]), (k, got[k], want[k])
    assert got["Bleu_1"] > got["Bleu_4"] > 0 and 0 < got["ROUGE_L"] < 1
    cm.reset()
    assert cm.sums is None and cm.compute()["images"] == 0
    cm.update(*batches[1])
    one = M.corpus(M.stats(*batches[1], 1, EOS, ce).tolist())
    assert all(close(cm.compute()[k], one[k]) for k in M.NAMES)


def test_caption_metrics_carries_cider():
    from klab_multimodalmodel_amd import metrics, scst
    table = scst.CiderD.from_references([[[5, 6, EOS]], [[7, 8, EOS]]], vocab_size=64)
    cm = metrics.CaptionMetrics(cider=table)
    assert list(cm.compute()) == list(M.NAMES) + ["CIDEr-D", "images"] and cm.compute()["CIDEr-D"] == 0.0
    with pytest.raises(ValueError):
        metrics.CaptionMetrics(cider="table")


# ---- validation ------------------------------------------------------------------------------------------------------------------------
def test_every_value_error():
    from klab_multimodalmodel_amd import metrics
    i64 = torch.int64
    hyp, refs = torch.zeros(4, 20, dtype=i64), torch.zeros(2, 3, 8, dtype=i64)
    assert tuple(metrics.caption_stats(hyp, refs).shape) == (2, 2, 16)
    bad = [(hyp.int(), refs), (hyp, refs.int()), (hyp.float(), refs), (hyp.view(2, 2, 20), refs), (hyp[0], refs), (hyp, refs[0]),
           (hyp.tolist(), refs), (hyp, refs.tolist()),
           (torch.zeros(4, 66, dtype=i64), refs), (hyp, torch.zeros(2, 3, 65, dtype=i64)), (hyp, torch.zeros(2, 17, 8, dtype=i64)),
           (hyp, torch.zeros(2, 0, 8, dtype=i64)), (hyp, torch.zeros(2, 3, 0, dtype=i64)), (torch.zeros(4, 0, dtype=i64), refs),
           (torch.zeros(5, 20, dtype=i64), refs), (torch.zeros(0, 20, dtype=i64), refs), (hyp, torch.zeros(0, 3, 8, dtype=i64)),
           (hyp, refs.to("meta"))]
    for h, r in bad:
        with pytest.raises(ValueError):
            metrics.caption_stats(h, r)
    for eos in (-1, 0xFFFF, 1.0, None, True):
        with pytest.raises(ValueError):
            metrics.caption_stats(hyp, refs, eos_token_id=eos)
        with pytest.raises(ValueError):
            metrics.CaptionMetrics(eos_token_id=eos)
    assert tuple(metrics.caption_stats(torch.zeros(4, 65, dtype=i64), torch.zeros(2, 16, 64, dtype=i64)).shape) == (2, 2, 16)  # the limits
    stats = metrics.caption_stats(hyp, refs)
    for s in (stats.double(), stats[..., :15], torch.tensor(3), stats.tolist()):
        with pytest.raises(ValueError):
            metrics.sentence_scores(s)
    for beta in (0.0, -1.0, math.nan, math.inf, "1.2"):
        with pytest.raises(ValueError):
            metrics.sentence_scores(stats, beta=beta)
    cm = metrics.CaptionMetrics()
    for h, r in ((hyp, refs), (hyp.view(2, 2, 20), refs), (hyp[:2].int(), refs), (hyp[:2], refs[:1])):
        with pytest.raises(ValueError):
            cm.update(h, r)
    assert cm.sums is None  # a refused update adds nothing


def test_reward_weights_validate():
    from klab_multimodalmodel_amd import scst
    from tests.test_scst_cpu import tiny_model
    m, _g = tiny_model()
    cfg = m.main_cfg
    table = scst.CiderD.from_references([[[5, 6, cfg.eos_token_id]]], vocab_size=cfg.vocab_size, eos_token_id=cfg.eos_token_id)
    assert scst.SelfCritical(m, table).reward_weights is None
    sc = scst.SelfCritical(m, table, reward_weights={"bleu4": 1})
    assert sc.reward_weights == {"ciderd": 0.0, "bleu4": 1.0, "rouge_l": 0.0}
    scst.SelfCritical(m, table, reward_weights={"ciderd": 1.0, "bleu4": 0.5, "rouge_l": -0.25})
    for bad in ({}, {"ciderd": 0.0}, {"ciderd": 0, "bleu4": 0.0}, {"meteor": 1.0}, {"ciderd": 1.0, "bleu_4": 0.5}, {"ciderd": math.nan},
                {"bleu4": math.inf}, {"ciderd": "1"}, {"ciderd": None}, [1.0, 0.5, 0.25], "ciderd", 1.0):
        with pytest.raises(ValueError):
            scst.SelfCritical(m, table, reward_weights=bad)


def test_entry_point_is_declared():
    from klab_multimodalmodel_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "klab_mm.h")).read()
    name, nargs = "klab_caption_stats", 11
    mt = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert mt, f"{name} is not declared in include/klab_mm.h"
    assert len(mt.group(1).split(",")) == nargs
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
    assert hasattr(_lib.load(), name), f"{name} is not exported by the built library"
    assert callable(ops.caption_stats)
