"""The tests' torch restatement of HF's logits processors (tests/logits_proc_ref.py) and MyModel.generate's argument handling
(klab_multimodalmodel_amd/logits_proc.py) against HF's own classes and generate, as stored by tests/golden/make_proc_goldens.py."""
import json
import os

import numpy as np
import pytest
import torch

from klab_multimodalmodel_amd.logits_proc import logits_processor_settings
from tests.helpers import GOLD
from tests.logits_proc_ref import EOS, generate_processors, hf_process


def _gold():
    return np.load(os.path.join(GOLD, "proc.npz")), json.load(open(os.path.join(GOLD, "proc.json")))


def _kw(p):
    return {k: p[k] for k in ("repetition_penalty", "no_repeat_ngram_size", "bad_words_ids", "min_length", "min_new_tokens")}


def test_restatement_matches_hf_processors():
    z, meta = _gold()
    xs, hs, outs = torch.from_numpy(z["pin_x"]), torch.from_numpy(z["pin_hist"]), torch.from_numpy(z["pin_out"])
    assert len(meta["pin"]) == xs.shape[0] >= 100
    banned = penalised = 0
    for i, p in enumerate(meta["pin"]):
        L = p["cur_len"]
        hist = hs[i, :, :L]
        got = hf_process(hist, xs[i], log_softmax=p["mode"] == "logprobs", **_kw(p))
        want = outs[i]
        assert torch.equal(torch.isinf(got), torch.isinf(want)), (i, p)
        fin = ~torch.isinf(want)
        assert torch.equal(got[fin], want[fin]), (i, p)
        base = torch.log_softmax(xs[i], -1) if p["mode"] == "logprobs" else xs[i]
        banned += int(torch.isinf(want).any())
        penalised += int((fin & (want != base)).any())
    assert banned > 40 and penalised > 20, (banned, penalised)  # the fixture exercises the bans and the penalty


def test_settings_match_hf_errors():
    _, meta = _gold()
    vocab = next(c["vocab"] for c in meta["cases"] if c["model"] == "tiny_a")
    assert len(meta["errors"]) >= 15
    for e in meta["errors"]:
        if e["type"] is None:
            logits_processor_settings(**e["kwargs"], eos_token_id=EOS, vocab_size=vocab)
            continue
        with pytest.raises(Exception) as info:
            logits_processor_settings(**e["kwargs"], eos_token_id=EOS, vocab_size=vocab)
        assert type(info.value).__name__ == e["type"] and str(info.value) == e["message"], (e, info.value)


def test_settings_fold_and_inactive():
    s = dict(eos_token_id=EOS, vocab_size=100)
    assert logits_processor_settings(**s) is None
    assert logits_processor_settings(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=1, min_new_tokens=None, **s) is None
    assert logits_processor_settings(min_new_tokens=0, min_length=7, **s) is None  # HF: min_length becomes 0 + 1
    got = logits_processor_settings(min_new_tokens=4, min_length=9, **s)
    assert got["min_length"] == 5 and got["min_new_tokens"] == 4
    got = logits_processor_settings(bad_words_ids=[[EOS], [3, 4], [np.int64(5)]], **s)
    assert got["bad_words_ids"] == [[3, 4], [5]]
    with pytest.raises(NotImplementedError):
        logits_processor_settings(bad_words_ids=[[2] * 1025], **s)


def _banned(hist, V, kw):
    return torch.isinf(hf_process(hist, torch.zeros(hist.shape[0], V), **kw))


def test_proc_goldens_are_consistent():
    z, meta = _gold()
    cases = meta["cases"]
    det = [c for c in cases if c["mode"] != "sample"]
    assert len(det) >= 60 and len(cases) - len(det) >= 40
    assert {c["procs"] for c in det} >= {"rep", "ngram2", "bad", "minlen", "minnew_minlen", "all"}
    assert any(c["procs"] == "minnew_minlen" and c["kwargs"]["min_length"] > c["kwargs"]["min_new_tokens"] + 1 for c in cases)
    for cs in cases:
        seq = torch.from_numpy(z[cs["id"] + ".seq"])
        assert (seq[:, 0] == 0).all() and seq.shape[1] <= cs["max_length"], cs["id"]
        kw = generate_processors(cs["kwargs"])
        kept = None
        if cs["mode"] == "sample":
            kept = np.unpackbits(z[cs["id"] + ".kept"], axis=-1)[..., :cs["vocab"]].astype(bool)
        # every emitted token through the row's EOS is one HF's processors allow at its step (the penalty bans nothing)
        for r in range(seq.shape[0]):
            for t in range(1, seq.shape[1]):
                if EOS in seq[r, 1:t].tolist():
                    break
                ban = _banned(seq[r:r + 1, :t], cs["vocab"], kw)[0]
                assert not ban[seq[r, t]], (cs["id"], r, t)
                if kept is not None:
                    assert kept[r, t - 1, seq[r, t]] and not (kept[r, t - 1] & ban.numpy()).any(), (cs["id"], r, t)
