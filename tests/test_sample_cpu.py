"""The tests' torch restatement of HF's sampling warpers (tests/sample_ref.py) against HF's own classes, as stored by
tests/golden/make_sample_goldens.py."""
import itertools
import json
import os

import numpy as np
import torch

from tests.helpers import GOLD
from tests.sample_ref import hf_warp, inverse_cdf


def test_restatement_matches_hf_warpers():
    z = np.load(os.path.join(GOLD, "sample.npz"))
    meta = json.load(open(os.path.join(GOLD, "sample.json")))["warp"]
    grid = list(itertools.product(meta["temperature"], meta["top_k"], meta["top_p"]))
    xs, outs = torch.from_numpy(z["warp_x"]), torch.from_numpy(z["warp_out"])
    assert outs.shape[:2] == (meta["matrices"], len(grid))
    removed_somewhere = 0
    for i in range(meta["matrices"]):
        for g, (t, k, p) in enumerate(grid):
            got = hf_warp(xs[i], t, k, p)
            want = outs[i, g]
            assert torch.equal(torch.isinf(got), torch.isinf(want)), (i, t, k, p)
            fin = ~torch.isinf(want)
            assert torch.equal(got[fin], want[fin]), (i, t, k, p)
            removed_somewhere += int(torch.isinf(want).any())
    assert removed_somewhere > len(grid)  # the fixture exercises the filters


def test_sample_goldens_are_consistent():
    z = np.load(os.path.join(GOLD, "sample.npz"))
    cases = json.load(open(os.path.join(GOLD, "sample.json")))["cases"]
    assert len(cases) >= 400
    for cs in cases:
        seq = z["seq"][cs["row0"]:cs["row0"] + cs["rows"], :cs["length"]]
        kept = np.unpackbits(z["kept"][cs["row0"]:cs["row0"] + cs["rows"], :cs["length"] - 1], axis=-1)[..., :cs["vocab"]]
        # every token HF sampled up to the row's EOS lies in its step's kept set (pads follow); top_k = 1 keeps one token
        tok = seq[:, 1:]
        live = np.cumsum(np.cumsum(tok == 1, 1), 1) <= 1  # through the first EOS
        hit = kept[np.arange(tok.shape[0])[:, None], np.arange(tok.shape[1])[None], tok]
        assert hit[live].all(), cs["id"]
        if cs["top_k"] == 1:
            assert (kept.sum(-1) == 1).mean() > 0.9, cs["id"]


def test_inverse_cdf_pick():
    w = torch.tensor([[0.0, -float("inf"), 0.0, float(np.log(2.0))]])
    # kept probabilities 1/4, 0, 1/4, 1/2 -> CDF steps 0.25, 0.5, 1.0 at ids 0, 2, 3
    for u, want in ((0.0, 0), (0.2, 0), (0.3, 2), (0.6, 3), (0.999, 3)):
        tok, dist = inverse_cdf(w, torch.tensor([u]))
        assert int(tok) == want, (u, tok)
    assert abs(float(inverse_cdf(w, torch.tensor([0.26]))[1]) - 0.01) < 1e-6
