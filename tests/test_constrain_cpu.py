"""Trie-constrained decoding, the part that needs no GPU: constrain.TokenTrie against a dict trie, the torch restatement of HF's
PrefixConstrainedLogitsProcessor against HF's own class (tests/golden/constrain.npz), the C struct mirrors, and the argument errors
of generate(constraint=...) that are raised before the engine."""
import ctypes as C
import json
import os
import random
import types

import numpy as np
import pytest
import torch

from tests.constrain_ref import EOS, DictTrie, hf_constrain, random_phrases, walk
from tests.helpers import GOLD, load_golden

V = 97


def _trie(sets, vocab=V, eos=EOS):
    from klab_multimodalmodel_amd.constrain import TokenTrie
    return TokenTrie.from_sequence_sets(sets, vocab, eos)


def _tables(t):
    return tuple(x.tolist() for x in (t.child_off, t.child_tok, t.child_node, t.roots))


def _prefixes(phrases, rng, n_off=20):
    """every prefix of every phrase (with its closing EOS and one pad behind it), and prefixes that leave the trie"""
    out = set()
    for p in phrases:
        q = list(p) + [EOS, 0]
        for i in range(len(q) + 1):
            out.add(tuple(q[:i]))
    for _ in range(n_off):
        p = rng.choice(phrases)
        out.add(tuple(p[:rng.randint(0, len(p))] + [rng.randrange(2, V)] * rng.randint(1, 2)))
    return sorted(out)


@pytest.mark.parametrize("n", [1, 2, 17, 300, 5000])
def test_trie_matches_dict_trie(n):
    rng = random.Random(n)
    phrases = random_phrases(rng, n, V)
    t = _trie([phrases])
    ref = DictTrie([phrases])
    off, tok, node, roots = _tables(t)
    assert t.n_sets == 1 and t.n_nodes == len(off) - 1 and t.n_edges == len(tok) == len(node) and off[0] == 0 and off[-1] == t.n_edges
    assert all(t.child_off.dtype == x.dtype == torch.int32 for x in (t.child_tok, t.child_node, t.roots))
    for i in range(t.n_nodes):
        seg = tok[off[i]:off[i + 1]]
        assert seg == sorted(set(seg)), i  # ascending, no duplicates
    assert sorted(node) == [i for i in range(t.n_nodes) if i != roots[0]]  # every node but the root has exactly one edge into it
    some = _prefixes(phrases if n <= 300 else rng.sample(phrases, 300), rng)
    for p in some:
        assert t.allowed(p) == ref.allowed(p), p
        assert t.contains(p) == ref.contains(p), p
        want = ref.node(p)
        assert (t.walk(p) >= 0) == (want is not None), p
        assert t.walk(p) == walk((off, tok, node, roots), p), p
    for p in phrases[:200]:
        assert t.contains(p) and t.contains(p + [EOS])
    assert ref.phrases() == sorted(p + [EOS] for p in phrases)


def test_trie_duplicates_prefixes_and_the_empty_phrase():
    a = _trie([[[5, 6], [5, 6, EOS], [5], [7, 8, 9], [5, 6]]])
    b = _trie([[[5], [5, 6], [7, 8, 9]]])
    assert _tables(a) == _tables(b)
    assert b.allowed([]) == [5, 7] and b.allowed([5]) == [EOS, 6] and b.allowed([5, 6]) == [EOS]
    assert b.allowed([5, EOS]) == [EOS] and b.allowed([5, EOS, 0]) == [EOS] and b.allowed([9]) == [EOS]
    assert b.contains([5]) and b.contains([5, 6]) and not b.contains([7, 8]) and not b.contains([]) and not b.contains([5, EOS, 6])
    assert b.n_nodes == 1 + 2 + 3 + 2 + 1 and b.n_edges == b.n_nodes - 1
    e = _trie([[[], [4]]])
    assert e.allowed([]) == [EOS, 4] and e.contains([]) and e.contains([EOS]) and e.contains([4])
    only = _trie([[[EOS]]])
    assert only.n_nodes == 2 and only.allowed([]) == [EOS]


def test_trie_sets_are_independent():
    rng = random.Random(3)
    sets = [random_phrases(rng, n, V) for n in (4, 60, 1)]
    t = _trie(sets)
    ref = DictTrie(sets)
    assert t.n_sets == 3 and len(set(t.roots.tolist())) == 3
    for s, phrases in enumerate(sets):
        for p in _prefixes(phrases, rng, 5):
            assert t.allowed(p, set=s) == ref.allowed(p, s), (s, p)
        other = (s + 1) % 3
        for p in phrases:
            assert t.contains(p, set=s) and t.contains(p, set=other) == ref.contains(p, other)
    one = _trie([sets[1]])
    assert one.n_nodes + _trie([sets[0]]).n_nodes + _trie([sets[2]]).n_nodes == t.n_nodes
    with pytest.raises(ValueError):
        t.allowed([], set=3)


def test_trie_state_dict_round_trip_and_to():
    from klab_multimodalmodel_amd.constrain import TokenTrie
    t = _trie([random_phrases(random.Random(1), 50, V), [[3]]])
    sd = t.state_dict()
    assert sd["vocab_size"] == V and sd["eos_token_id"] == EOS
    u = TokenTrie.from_state_dict(sd)
    assert _tables(u) == _tables(t) and (u.vocab_size, u.eos_token_id, u.n_sets) == (V, EOS, 2)
    assert u.to("cpu") is u and u.device == torch.device("cpu")
    sd["child_node"] = sd["child_node"] + t.n_nodes
    with pytest.raises(ValueError):
        TokenTrie.from_state_dict(sd)


def test_trie_value_errors():
    from klab_multimodalmodel_amd.constrain import TokenTrie
    for bad in ([[5, EOS, 6]], [[EOS, 5]], [[5, V]], [[-1]], []):
        with pytest.raises(ValueError):
            TokenTrie.from_sequences(bad, V, EOS)
    with pytest.raises(ValueError):
        TokenTrie.from_sequence_sets([[[5]], []], V, EOS)
    with pytest.raises(ValueError):
        TokenTrie.from_sequence_sets([], V, EOS)
    with pytest.raises(ValueError):
        TokenTrie.from_sequences([[5]], V, V)


def test_restatement_matches_hf_processor():
    z = np.load(os.path.join(GOLD, "constrain.npz"))
    meta = json.load(open(os.path.join(GOLD, "constrain.json")))
    pin = meta["pin"]
    trie = DictTrie(pin["phrase_sets"])
    x, hist, out = (torch.from_numpy(z[k]) for k in ("pin_x", "pin_hist", "pin_out"))
    assert len(pin["cases"]) == x.shape[0] >= 100 and {c["num_beams"] for c in pin["cases"]} == {1, 3}
    masked = 0
    for i, cs in enumerate(pin["cases"]):
        got = hf_constrain(x[i], hist[i, :, :cs["cur_len"]], trie, cs["sets"], cs["num_beams"])
        assert torch.equal(got, out[i]), i
        masked += int(torch.isinf(got).sum())
    assert masked > 0
    # ... and the package's trie answers the callback's question the same way
    t = _trie(pin["phrase_sets"], vocab=x.shape[-1])
    for i, cs in enumerate(pin["cases"]):
        for r in range(hist.shape[1]):
            h = hist[i, r, 1:cs["cur_len"]].tolist()
            s = cs["sets"][r // cs["num_beams"]]
            assert t.allowed(h, set=s) == trie.allowed(h, s)


def test_c_mirrors_have_the_c_sizes():
    from klab_multimodalmodel_amd import _lib as L
    from klab_multimodalmodel_amd import engine
    lib = L.load()
    assert lib.klab_sizeof_constrain_args() == C.sizeof(L.ConstrainArgs)
    assert lib.klab_sizeof_gen_cfg() == C.sizeof(L.GenCfg)
    assert "klab_constrain_rows" in L.SIGNATURES and hasattr(lib, "klab_constrain_rows")
    # the constraint is armed by a setter, as the forced table and the maps are: klab_gen_cfg keeps its fields and its size
    assert "klab_engine_gen_set_constraint" in engine.ENGINE_SIGS and hasattr(lib, "klab_engine_gen_set_constraint")
    assert "constraint" not in [f[0] for f in L.GenCfg._fields_]
    cfg = engine.Engine.gen_cfg("pick", 1, 7, 1, 0)
    assert cfg.constraint is None
    t = _trie([[[5], [6, 7]]])
    roots = t.roots[torch.zeros(3, dtype=torch.int64)].contiguous()
    cfg = engine.Engine.gen_cfg("beam", 2, 7, 1, 0, constraint=(t, roots))
    k = cfg.constraint
    assert (k.n_nodes, k.n_edges, k.child_off, k.root_dev) == (t.n_nodes, t.n_edges, t.child_off.data_ptr(), roots.data_ptr())
    with pytest.raises(ValueError):
        engine.Engine.gen_cfg("pick", 1, 7, 1, 0, constraint=(t, roots.long()))


def _model():
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_golden("tiny_b")
    sw = SwinConfig.from_dict(g["meta"]["swin_config"])
    t5 = T5Config.from_dict(g["meta"]["t5_config"])
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], g["sds"]["main"]), dtype="fp32")
    return m, g["inputs"]["pixel_values"], g["inputs"]["src_ids"]


def test_generate_constraint_argument_errors():
    m, pix, src = _model()
    vocab, B = m.main_cfg.vocab_size, src.shape[0]
    good = _trie([[[5], [6, 7]], [[8]]], vocab=vocab)
    with pytest.raises(ValueError, match="needs `constraint`"):
        m.generate(pix, src, constraint_set=[0] * B)
    with pytest.raises(ValueError, match="TokenTrie"):
        m.generate(pix, src, constraint=[[5]])
    with pytest.raises(ValueError, match="vocab_size"):
        m.generate(pix, src, constraint=_trie([[[5]]], vocab=vocab - 1))
    with pytest.raises(ValueError, match="eos_token_id"):
        m.generate(pix, src, constraint=_trie([[[5]]], vocab=vocab, eos=2))
    with pytest.raises(ValueError, match="trie is on"):
        m.generate(pix, src.to("meta"), constraint=good)
    with pytest.raises(ValueError, match="kv_cache=True"):
        m.generate(pix, src, constraint=good, kv_cache=False)
    for bad in ([0] * (B + 1), [[0] * B], [0.0] * B, [2] + [0] * (B - 1), [-1] + [0] * (B - 1)):
        with pytest.raises(ValueError, match="constraint_set"):
            m.generate(pix, src, constraint=good, constraint_set=bad)
    with pytest.raises(ValueError, match="constraint_set"):
        m.generate(pix, src, num_beams=2, constraint=good, constraint_set=torch.zeros(B, 1, dtype=torch.int64))
