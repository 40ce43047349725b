"""What tests/test_scst_gpu.py takes for granted, proved without a GPU: known values of the CIDEr-D reference of tests/scst_ref.py,
the idf table of scst.CiderD.from_references against the Counter statement and the numpy probe (wrapped chains included), the
reward tolerance as derived, the targets reference on a case done by hand, and the validation errors of from_references,
SelfCritical and weight_norm."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import scst_ref as S
from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = S.EOS


def one_image(hyp, refs, corpus=None, **kw):
    corpus = [[r + [EOS] for r in refs]] if corpus is None else corpus
    df = S.doc_freq(corpus)
    return float(S.reward(S.units(hyp + [EOS]), [S.units(r + [EOS]) for r in refs], df, max(len(corpus), 1), **kw))


# ---- known values ------------------------------------------------------------------------------------------------------------------------
# (a corpus of ONE image gives idf = log 1 - log 1 = 0 for its own n-grams, so these use a corpus that does not hold them: idf = log N)
OTHER = [[[30, 31, EOS]], [[32, 33, EOS]], [[34, EOS]]]


def test_a_hypothesis_equal_to_its_only_reference_scores_ten():
    for cap in ([5, 6, 7], [5, 6, 7, 8, 9, 10], [5, 5, 5, 5, 6]):  # (with EOS: >= 4 units)
        assert abs(one_image(cap, [cap], OTHER) - 10.0) <= 1e-12


def test_three_units_score_seven_and_a_half():
    assert abs(one_image([5, 6], [[5, 6]], OTHER) - 7.5) <= 1e-12  # 5, 6, EOS: orders 1..3 score 1, order 4 has no n-gram


def test_disjoint_sequences_score_exactly_zero():
    df = S.doc_freq(OTHER)
    assert float(S.reward([5, 6, 7, 8], [[9, 10, 11, 12]], df, 3)) == 0.0
    assert float(S.reward([], [[9, 10]], df, 3)) == 0.0 and float(S.reward([5], [], df, 3)) == 0.0


def test_the_length_penalty_by_hand():
    # hypothesis a, reference a a (no EOS, count_eos off), idf = L = log 3 everywhere.  Order 1: vec_h = L, vec_r = 2 L,
    # min(L, 2 L) 2 L / (L 2 L) = 1, times exp(-1 / 72); orders 2..4: the hypothesis has no n-gram.
    df = S.doc_freq(OTHER)
    got = float(S.reward([5], [[5, 5]], df, 3, sigma=6.0))
    assert abs(got - 10.0 * math.exp(-1.0 / 72.0) / 4.0) <= 1e-12
    # ... and the clip: hypothesis a a a against reference a: min(3 L, L) L / (3 L L) = 1 / 3, times exp(-4 / 72)
    got = float(S.reward([5, 5, 5], [[5]], df, 3, sigma=6.0))
    assert abs(got - 10.0 * (math.exp(-4.0 / 72.0) / 3.0) / 4.0) <= 1e-12


def test_document_frequency_counts_images_not_references():
    corpus = [[[5, 6, EOS], [5, 6, EOS], [5, 6, 7, EOS]], [[5, EOS]], [[8, EOS]]]
    df = S.doc_freq(corpus)
    assert df[(5, 6)] == 1 and df[(5,)] == 2 and df[(EOS,)] == 3 and df[(8, EOS)] == 1
    from klab_multimodalmodel_amd import scst
    t = scst.CiderD.from_references(corpus, vocab_size=16)
    keys = t.keys.numpy().view(np.uint64)
    v, slot, _p = S.table_lookup(keys, t.idf.numpy(), S.gram_key((5, 6)), t.log_n)
    assert slot >= 0 and v == float(np.float32(math.log(3) - math.log(1)))
    v, slot, _p = S.table_lookup(keys, t.idf.numpy(), S.gram_key((5,)), t.log_n)
    assert slot >= 0 and v == float(np.float32(math.log(3) - math.log(2)))


def test_units_rule():
    assert S.units([5, 6, EOS, 7]) == [5, 6, EOS] and S.units([5, 6, EOS, 7], count_eos=False) == [5, 6]
    assert S.units([5, -100, 6]) == [5] and S.units([5, 0xFFFF, 6]) == [5] and S.units([5, 0xFFFE]) == [5, 0xFFFE]
    assert S.units([EOS]) == [EOS] and S.units([EOS], count_eos=False) == []


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def build_table(c):
    from klab_multimodalmodel_amd import scst
    cap = None
    if c["capacity"] == "smallest":
        cap = S.smallest_capacity(len(S.doc_freq(c["corpus"], EOS, c["count_eos"])))
    return scst.CiderD.from_references(c["corpus"], vocab_size=c["V"], eos_token_id=EOS, count_eos=c["count_eos"], capacity=cap)


@pytest.mark.parametrize("name", list(S.reward_cases()))
def test_every_key_is_found_with_its_idf_and_absent_keys_give_log_n(name):
    c = S.reward_cases()[name]
    df = S.doc_freq(c["corpus"], EOS, c["count_eos"])
    t = build_table(c)
    N = len(c["corpus"])
    keys, idf = t.keys.numpy().view(np.uint64), t.idf.numpy()
    cap = len(keys)
    assert t.entries == len(df) and cap & (cap - 1) == 0 and cap >= 2 * len(df) and t.n_images == N
    assert int((keys != np.uint64(S.EMPTY)).sum()) == len(df)
    assert t.log_n == float(np.float32(math.log(N)))
    wrapped = 0
    for g, d in df.items():
        k = S.gram_key(g)
        v, slot, _p = S.table_lookup(keys, idf, k, t.log_n)
        assert slot >= 0 and v == float(np.float32(math.log(N) - math.log(d))), (g, v)
        wrapped += slot < S.home_slot(k, cap)
    for g in ((40,), (40, 41), (2, 40, 2), (40, 41, 40, 41), (0xFFFE, 0xFFFE, 0xFFFE, 0xFFFE)):
        if g not in df:
            assert S.table_lookup(keys, idf, S.gram_key(g), t.log_n) == (t.log_n, -1, 0)
    if c["capacity"] == "smallest":
        assert cap == S.smallest_capacity(len(df)) and wrapped >= 1, "no probe chain wraps around the end of this table"


def test_a_full_chain_is_bounded_by_the_capacity():
    keys = np.array([5, 6], dtype=np.uint64)  # no empty slot: the probe of an absent key ends after cap steps
    assert S.table_lookup(keys, np.zeros(2, np.float32), 7, 1.5) == (1.5, -1, 0)


def test_state_dict_round_trip():
    from klab_multimodalmodel_amd import scst
    t = build_table(S.reward_cases()["batch count_eos=False"])
    u = scst.CiderD.from_state_dict(t.state_dict())
    assert torch.equal(t.keys, u.keys) and torch.equal(t.idf, u.idf)
    for a in ("n_images", "entries", "vocab_size", "eos_token_id", "count_eos", "sigma", "log_n", "capacity"):
        assert getattr(t, a) == getattr(u, a), a
    assert u.count_eos is False and u.to("cpu") is u


def test_the_reward_tolerance_is_the_derived_one():
    worst = 0.0
    for c in S.reward_cases().values():
        worst = max(worst, float(np.abs(S.case_reference(c, fp32=True) - S.case_reference(c)).max()))
    print("largest |fp32 mode - fp64 mode| over the fixture set:", worst)
    assert S.REWARD_TOL_FACTOR == 8.0 and S.REWARD_TOL == S.REWARD_TOL_FACTOR * worst
    assert 0 < S.REWARD_TOL < 1e-4  # a bound that is no tolerance in disguise: rewards reach 10


def test_the_fixture_set_holds_what_the_gpu_test_relies_on():
    cases = S.reward_cases()
    lens = {ce: [len(S.units(r[1:], EOS, ce)) for r in cases[f"lengths count_eos={ce}"]["hyp"].tolist()] for ce in (True, False)}
    assert lens[True] == [1, 3, 4, 63, 64] and lens[False] == [1, 3, 4, 63, 64]
    assert EOS not in cases["lengths count_eos=False"]["hyp"][4].tolist()  # 64 units without an EOS
    b = cases["batch count_eos=True"]
    assert tuple(b["hyp"].shape) == (15, 20) and tuple(b["refs"].shape) == (3, 5, 16) and b["n_h"] == 5
    assert bool((b["refs"][2, :, 0] < 0).all()) and int((b["refs"][1, :, 0] < 0).sum()) == 2
    assert b["hyp"][0, 1] == EOS and EOS not in b["hyp"][1].tolist()
    want = S.case_reference(b)
    assert bool((want[10:] == 0).all()) and bool((want[5:10] > 0).any())
    assert float(S.case_reference(cases["batch count_eos=False"])[0]) == 0.0  # EOS first and not counted: no units
    assert int((cases["sixteen references"]["refs"][0, :, 0] < 0).sum()) == 3 and cases["sixteen references"]["refs"].shape[1] == 16
    e = cases["extreme ids"]
    assert int(e["hyp"].max()) == e["V"] - 1 == 65534 and int(e["hyp"].min()) == 0
    assert (40, 41) not in S.doc_freq(e["corpus"]) and bool((S.case_reference(e) > 0).all())
    one = S.case_reference(cases["one reference"])
    assert abs(one[0] - 10.0) <= 1e-12


# ---- targets -----------------------------------------------------------------------------------------------------------------------------
def test_targets_reference_by_hand():
    seq = torch.tensor([[0, 5, 6, EOS, 0], [0, 7, 8, 9, 10]])
    rew = torch.tensor([0.5, 2.0])
    lab, w, adv = S.targets(seq, rew, None, 1, 2, 6)
    assert lab.tolist() == [[5, 6, EOS, -100, -100, -100], [7, 8, 9, 10, -100, -100]]
    assert adv.tolist() == [-1.5, 1.5]
    assert w.tolist() == [[-1.5] * 3 + [0.0] * 3, [1.5] * 4 + [0.0] * 2]
    assert S.targets(seq, rew, torch.tensor([0.25]), 0, 2, 4)[2].tolist() == [0.25, 1.75]
    assert S.targets(seq, rew, None, 2, 1, 4)[2].tolist() == [0.5, 2.0]


# ---- validation ------------------------------------------------------------------------------------------------------------------------
def test_from_references_validates():
    from klab_multimodalmodel_amd import scst
    good = [[[5, 6, EOS]], [[7, EOS]]]
    entries = len(S.doc_freq(good))
    for kw in (dict(vocab_size=65536), dict(vocab_size=0), dict(vocab_size=6), dict(vocab_size=16, eos_token_id=16),
               dict(vocab_size=16, sigma=0.0), dict(vocab_size=16, sigma=math.nan), dict(vocab_size=16, capacity=entries),
               dict(vocab_size=16, capacity=2 * entries - 1 if (2 * entries - 1) & (2 * entries - 2) else 3),
               dict(vocab_size=16, capacity=S.smallest_capacity(entries) // 2)):
        with pytest.raises(ValueError):
            scst.CiderD.from_references(good, **kw)
    with pytest.raises(ValueError):
        scst.CiderD.from_references([], vocab_size=16)
    with pytest.raises(ValueError):
        scst.CiderD.from_references([[list(range(2, 12)) * 7]], vocab_size=16)  # 70 units
    t = scst.CiderD.from_references(good, vocab_size=16, capacity=4 * S.smallest_capacity(entries))
    assert t.capacity == 4 * S.smallest_capacity(entries) and t.entries == entries
    assert scst.CiderD.from_references([[], [[5, EOS]]], vocab_size=16).n_images == 2  # an image without references still counts


def tiny_model():
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_golden("tiny_a")
    sw, t5 = SwinConfig.from_dict(g["meta"]["swin_config"]), T5Config.from_dict(g["meta"]["t5_config"])
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    return MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], g["sds"]["main"]), dtype=torch.float32), g


def test_weight_norm_validates_and_reads_back():
    m, _g = tiny_model()
    assert m.loss_options == {"label_smoothing": 0.0, "z_loss": 0.0}
    m.set_loss_options(label_smoothing=0.1, weight_norm="count")
    assert m.loss_options == {"label_smoothing": 0.1, "z_loss": 0.0, "weight_norm": "count"}
    for bad in ("mean", None, 1, "COUNT"):
        with pytest.raises(ValueError):
            m.set_loss_options(weight_norm=bad)
        assert m.loss_options == {"label_smoothing": 0.1, "z_loss": 0.0, "weight_norm": "count"}  # a refused call changes nothing
    m.set_loss_options(label_smoothing=0.1)
    assert m.loss_options == {"label_smoothing": 0.1, "z_loss": 0.0}
    assert not any("weight_norm" in k for k in m.state_dict())


def test_self_critical_validates_before_anything_runs():
    from klab_multimodalmodel_amd import scst
    m, g = tiny_model()
    cfg = m.main_cfg
    table = scst.CiderD.from_references([[[5, 6, cfg.eos_token_id]]], vocab_size=cfg.vocab_size, eos_token_id=cfg.eos_token_id)
    scst.SelfCritical(m, table, samples=1, baseline="greedy")
    scst.SelfCritical(m, table, samples=2, baseline="mean", max_length=65)
    for kw in (dict(samples=1, baseline="mean"), dict(samples=0), dict(samples=2.0), dict(baseline="best"), dict(max_length=66),
               dict(max_length=1)):
        with pytest.raises(ValueError):
            scst.SelfCritical(m, table, **kw)
    other = scst.CiderD.from_references([[[5, 6, 1]]], vocab_size=cfg.vocab_size - 1, eos_token_id=cfg.eos_token_id)
    with pytest.raises(ValueError):
        scst.SelfCritical(m, other)
    with pytest.raises(ValueError):
        scst.SelfCritical(m, "table")
    sc = scst.SelfCritical(m, table, samples=2)
    inp = g["inputs"]
    B = inp["src_ids"].shape[0]
    assert B >= 2  # (B + 1 rows below are then no multiple of B)
    images, source = {"pixel_values": inp["pixel_values"]}, {"input_ids": inp["src_ids"]}
    for refs in (torch.zeros(B, 2, 8), torch.zeros(B, 2, dtype=torch.int64), torch.zeros(B + 1, 2, 8, dtype=torch.int64),
                 torch.zeros(B, 17, 8, dtype=torch.int64), torch.zeros(B, 2, 65, dtype=torch.int64), [[[5, 6, 1]]] * B):
        with pytest.raises(ValueError):
            sc.loss(images, source, refs)
    with pytest.raises(ValueError):
        scst.ciderd(table, torch.zeros(B, 66, dtype=torch.int64), torch.zeros(B, 2, 8, dtype=torch.int64))
    with pytest.raises(ValueError):
        scst.ciderd(table, torch.zeros(B + 1, 20, dtype=torch.int64), torch.zeros(B, 2, 8, dtype=torch.int64))
    assert m.loss_options == {"label_smoothing": 0.0, "z_loss": 0.0}


def test_entry_points_are_declared():
    from klab_multimodalmodel_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "klab_mm.h")).read()
    for name, nargs in (("klab_ciderd_rewards", 16), ("klab_scst_targets", 13), ("klab_engine_set_weight_norm", 2),
                        ("klab_engine_set_loss_options", 4)):
        mt = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert mt, f"{name} is not declared in include/klab_mm.h"
        assert len(mt.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(_lib.load(), name), f"{name} is not exported by the built library"
    assert callable(ops.ciderd_rewards) and callable(ops.scst_targets)
