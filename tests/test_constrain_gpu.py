"""Trie-constrained decoding on the device: klab_constrain_rows (csrc/constrain.hip) against the torch restatement of HF's
PrefixConstrainedLogitsProcessor and the host walk (tests/constrain_ref.py), MyModel.generate(constraint=...) against HF's own
generate with a prefix_allowed_tokens_fn as the reference runs it (tests/golden/constrain.npz from make_constrain_goldens.py),
and cross-checks that need no golden in all three loops."""
import ctypes as C
import functools
import json
import math
import os
import random

import numpy as np
import pytest
import torch

from tests.constrain_ref import EOS, DictTrie, hf_constrain, walk
from tests.helpers import GOLD
from tests.sample_ref import boundary_tokens
from tests.test_logits_proc_gpu import _configs1_model, _engine_kw, process_rows
from tests.test_sample_gpu import _build, _eos_row, _teacher_forced_logits, sample_rows

pytestmark = pytest.mark.gpu
NEG = -float("inf")


def _lib():
    from klab_multimodalmodel_amd import _lib as L
    return L, L.load()


def _trie(sets, vocab, device="cuda"):
    from klab_multimodalmodel_amd.constrain import TokenTrie
    return TokenTrie.from_sequence_sets(sets, vocab, EOS).to(device)


def _tables(t):
    return tuple(x.tolist() for x in (t.child_off, t.child_tok, t.child_node, t.roots))


def constrain_rows(x, t, node_in=None, last_tok=None, parent=None, roots=None, root_div=1, row_div=1, log_softmax=False, out=None,
                   V=None, eos_id=EOS):
    """klab_constrain_rows over x ([R, >= V] fp32 / bf16, device) for rows = R * row_div; the first position when roots is given
    (int32 [rows / root_div]), else an advance from node_in over last_tok.  out: the f32 buffer to write (default: a NaN-filled
    [rows, V + 5]).  Returns (node_out [rows], out) on the host."""
    L, lib = _lib()
    V = V or x.shape[-1]
    rows = x.shape[0] * row_div
    if out is None:
        out = torch.full((rows, V + 5), float("nan"), device="cuda")
    dev = lambda v, dt: None if v is None else torch.as_tensor(v, dtype=dt).cuda()  # noqa: E731
    nin, tok, par, rt = dev(node_in, torch.int32), dev(last_tok, torch.int64), dev(parent, torch.int32), dev(roots, torch.int32)
    nout = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    a = L.ConstrainArgs()
    a.dtype, a.logits, a.ld, a.row_div, a.rows, a.V, a.log_softmax = L.dtype_code(x.dtype), x.data_ptr(), x.stride(0), row_div, rows, V, int(log_softmax)
    a.child_off, a.child_tok, a.child_node, a.n_nodes, a.n_edges = t.child_off.data_ptr(), t.child_tok.data_ptr(), t.child_node.data_ptr(), t.n_nodes, t.n_edges
    a.first, a.root, a.root_div = int(roots is not None), L.ptr(rt), root_div
    a.node_in, a.parent, a.last_tok, a.node_out = L.ptr(nin), L.ptr(par), L.ptr(tok), nout.data_ptr()
    a.eos_id, a.out, a.ld_out = eos_id, out.data_ptr(), out.stride(0)
    L.check(lib.klab_constrain_rows(C.byref(a), L.stream_ptr()), "klab_constrain_rows")
    torch.cuda.synchronize()
    return nout.cpu(), out.cpu()


def _kernel_case(V):
    """phrases [a_i, t]: node a_i has exactly the children S_i -- every degree and child id of interest that fits V -- and the
    histories (behind the start token) whose last step the kernel takes"""
    rng = random.Random(V)
    must = [0, 31, 32, V - 1]
    degrees = [d for d in (1, 2, 63, 64, 65, 4097) if d < V - 8] + [V]
    phrases, hists = [], []
    for i, d in enumerate(degrees):
        a = 2 + i
        if d == V:
            kids = list(range(V))
        else:
            kids = set(rng.sample(must, min(d, len(must))))
            while len(kids) < d:
                kids.add(rng.randrange(V))
            kids = sorted(kids)
        phrases += [[a] if k == EOS else [a, k] for k in kids]
        hists.append([a])
    two = next(p for p in phrases if len(p) == 2)
    # an inner node, a leaf, behind a leaf (-1), -1 staying -1, and two tokens that are no child
    hists += [two, two + [EOS], two + [EOS, 0], two + [EOS, 0, 0], [2, EOS], [V - 2 if V > 40 else 20]]
    hists += [hists[0]] * (-len(hists) % 3)  # (a multiple of 3 for row_div)
    return phrases, hists


@functools.lru_cache(maxsize=None)
def _kernel_setup(V):
    phrases, hists = _kernel_case(V)
    t = _trie([phrases], V)
    ref = DictTrie([phrases])
    tab = _tables(t)
    node_in = [walk(tab, h[:-1]) for h in hists]
    want_node = [walk(tab, h) for h in hists]
    assert -1 in want_node and -1 in node_in and any(t.allowed(h) == [EOS] and n >= 0 for h, n in zip(hists, want_node))
    return t, ref, hists, node_in, want_node


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("V", [33, 384, 32128, 32768])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_constrain_rows_matches_restatement(V, dtype):
    t, ref, hists, node_in, want_node = _kernel_setup(V)
    rows = len(hists)
    g = torch.Generator().manual_seed(V)
    last = [h[-1] for h in hists]
    for row_div in (1, 3):
        x = (torch.randn(rows // row_div, V, generator=g) * 3.0).to(dtype)
        xf = x.float().repeat_interleave(row_div, 0)
        want = torch.stack([hf_constrain(xf[r:r + 1], torch.tensor([[0] + hists[r]]), ref, [0], 1)[0] for r in range(rows)])
        node, out = constrain_rows(x.cuda(), t, node_in=node_in, last_tok=last, row_div=row_div)
        assert node.tolist() == want_node, (V, dtype, row_div)
        # allowed entries are the input's fp32 value bit for bit, all others -inf, the columns behind V keep their NaN bits
        assert torch.equal(_bits(out[:, :V]), _bits(want)), (V, dtype, row_div)
        assert torch.equal(_bits(out[:, V:]), _bits(torch.full((rows, 5), float("nan")))), (V, dtype, row_div)
        # log_softmax over the WHOLE row: the bits klab_logits_process_rows gives
        lsm, _ = process_rows(x.cuda(), torch.zeros(rows, 1, dtype=torch.int64), row_div=row_div, log_softmax=True)
        _, out = constrain_rows(x.cuda(), t, node_in=node_in, last_tok=last, row_div=row_div, log_softmax=True)
        allowed = ~torch.isinf(want)
        assert torch.equal(torch.isinf(out[:, :V]), ~allowed) and (out[:, :V][~allowed] == NEG).all()
        assert torch.equal(_bits(out[:, :V][allowed]), _bits(lsm[allowed])), (V, dtype, row_div)
    # in place: out is the f32 input itself
    x = torch.randn(rows, V, generator=g) * 3.0
    buf = x.clone().cuda()
    want = torch.stack([hf_constrain(x[r:r + 1], torch.tensor([[0] + hists[r]]), ref, [0], 1)[0] for r in range(rows)])
    node, out = constrain_rows(buf, t, node_in=node_in, last_tok=last, out=buf)
    assert node.tolist() == want_node and torch.equal(_bits(out), _bits(want))


def test_constrain_rows_advance():
    V = 384
    rng = random.Random(9)
    from tests.constrain_ref import random_phrases
    sets = [random_phrases(rng, n, V) for n in (40, 7, 300)]
    t = _trie(sets, V)
    tab = _tables(t)
    x = torch.randn(12, V).cuda()
    # the first position: every row starts at the root of its image's set
    for root_div, which in ((1, [rng.randrange(3) for _ in range(12)]), (3, [2, 0, 1, 2])):
        roots = [tab[3][s] for s in which]
        node, out = constrain_rows(x, t, roots=roots, root_div=root_div)
        assert node.tolist() == [roots[r // root_div] for r in range(12)]
        for r in range(12):
            assert torch.nonzero(~torch.isinf(out[r, :V])).flatten().tolist() == t.allowed([], set=which[r // root_div])
    # an advance through a parent permutation with repeats: row r continues the row parent[r] stood on
    prefixes = [p[:rng.randint(0, len(p))] for p in rng.sample(sets[0], 12)]
    node_in = [walk(tab, p) for p in prefixes]
    node_in[5] = -1
    parent = [3, 3, 0, 7, 7, 5, 11, 1, 2, 2, 9, 0]
    last = []
    for r, par in enumerate(parent):
        kids = t.allowed(prefixes[par])
        last.append(kids[rng.randrange(len(kids))] if r % 3 else rng.randrange(V))  # every third row: any token, mostly no child
    want = [-1 if node_in[par] < 0 else walk(tab, prefixes[par] + [last[r]]) for r, par in enumerate(parent)]
    assert -1 in want and any(w >= 0 for w in want)
    node, _ = constrain_rows(x, t, node_in=node_in, last_tok=last, parent=parent)
    assert node.tolist() == want
    # -1 stays -1, and EOS leads to a leaf that allows only EOS
    p = sets[1][0]
    node, out = constrain_rows(x[:2], t, node_in=[-1, walk(tab, p, 1)], last_tok=[p[0], EOS])
    leaf = walk(tab, p + [EOS], 1)
    assert node.tolist() == [-1, leaf] and leaf >= 0 and tab[0][leaf] == tab[0][leaf + 1]
    assert all(torch.nonzero(~torch.isinf(out[r, :V])).flatten().tolist() == [EOS] for r in range(2))


def test_constrain_rows_rejects_oversized_and_bad_arguments():
    t = _trie([[[5], [6, 7]]], 32769)
    with pytest.raises(NotImplementedError):
        constrain_rows(torch.zeros(1, 32769, device="cuda"), t, roots=[0])
    t = _trie([[[5], [6, 7]]], 64)
    x = torch.zeros(2, 64, device="cuda")
    with pytest.raises(ValueError):
        constrain_rows(x, t)  # neither roots nor a state to advance
    with pytest.raises(ValueError):
        constrain_rows(x, t, roots=[0, 0], V=65)  # ld < V
    with pytest.raises(ValueError):
        constrain_rows(x, t, roots=[0, 0], out=torch.zeros(2, 63, device="cuda"))  # ld_out < V


# ---- generate against HF's generate ----------------------------------------------------------------------------------------------
def _gold():
    return np.load(os.path.join(GOLD, "constrain.npz")), json.load(open(os.path.join(GOLD, "constrain.json")))


def _getter(meta):
    models, tries = {}, {}

    def get(cs):
        key = (cs["model"], cs["variant"])
        if key not in models:
            models[key] = _build(cs["model"], "fp32", _eos_row(cs["model"]) if cs["variant"] == "eos" else None)
        tk = tuple(cs["sets"])
        if tk not in tries:
            sets = [meta["sets"][s] for s in tk]
            tries[tk] = (_trie(sets, cs["vocab"]), DictTrie(sets))
        return models[key] + tries[tk]
    return get


def _case_kw(z, cs, trie):
    kw = dict(cs["kwargs"], max_length=cs["max_length"], constraint=trie, constraint_set=cs["constraint_set"])
    if cs["prompt"]:
        kw["decoder_input_ids"] = torch.from_numpy(z[cs["model"] + ".prompt"])
    return kw


def test_generate_greedy_and_beam_match_reference():
    z, meta = _gold()
    cases = [c for c in meta["cases"] if c["mode"] != "sample"]
    assert len(cases) >= 30
    get = _getter(meta)
    for cs in cases:
        m, g, trie, _ = get(cs)
        pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
        want = torch.from_numpy(z[cs["id"] + ".seq"])
        kw = _case_kw(z, cs, trie)
        if cs["mode"] == "greedy":
            got = m.generate(pix, src, **kw).cpu()
            assert torch.equal(got, want), (cs["id"], got, want)
        else:
            got, sc = m.generate(pix, src, num_beams=cs["num_beams"], return_scores=True, **kw)
            assert torch.equal(got.cpu(), want), (cs["id"], got, want)
            ws = torch.from_numpy(z[cs["id"] + ".scores"])
            assert torch.allclose(sc.cpu(), ws, atol=1e-4, rtol=0), (cs["id"], sc, ws)


def _step_kept(logits, seq, t, kw, ref, which, skip, temperature, top_k):
    """the kept set of the token at position t + 1: processors, the restated constraint, then the warpers"""
    proc, _ = process_rows(logits[:, t].contiguous().cuda(), seq[:, :t + 1], **kw)
    proc = hf_constrain(proc, seq[:, :t + 1], ref, which, 1, skip=skip)
    _, warped = sample_rows(proc.cuda(), temperature, top_k, 1.0, u=torch.zeros(proc.shape[0], device="cuda"))
    return proc, ~torch.isinf(warped)


def test_generate_sample_matches_reference_kept_sets():
    z, meta = _gold()
    cases = [c for c in meta["cases"] if c["mode"] == "sample"]
    assert len(cases) >= 15
    get = _getter(meta)
    boundary = own = 0
    for cs in cases:
        m, g, trie, ref = get(cs)
        pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
        seq = torch.from_numpy(z[cs["id"] + ".seq"])
        V, t_, k_, which = cs["vocab"], cs.get("temperature", 1.0), cs["top_k"], cs["constraint_set"]
        want = np.unpackbits(z[cs["id"] + ".kept"], axis=-1)[..., :V].astype(bool)
        skip = seq.shape[1] - want.shape[1]  # the start token and the prompt: the first chosen position
        kw = _engine_kw(cs["kwargs"])
        if cs["prompt"] and kw.get("min_new_tokens"):
            kw["min_new_tokens"] += skip - 1
        lg = _teacher_forced_logits(m, pix, src, seq, 1)
        live = torch.from_numpy(np.cumsum(np.cumsum(seq[:, skip:].numpy() == EOS, 1), 1) <= 1)
        for i in range(want.shape[1]):
            proc, got = _step_kept(lg, seq, skip - 1 + i, kw, ref, which, skip, t_, k_)
            diff = (got != torch.from_numpy(want[:, i])) & live[:, i:i + 1]
            if diff.any():
                ok = boundary_tokens(proc, t_, k_, 1.0)
                assert not (diff & ~ok).any(), (cs["id"], i, torch.nonzero(diff & ~ok)[:8])
                boundary += int(diff.any(-1).sum())
        # our own generate: every emitted token (through its row's EOS) lies in its step's kept set
        torch.manual_seed(own)
        own += 1
        ours = m.generate(pix, src, do_sample=True, temperature=t_, top_k=k_, **_case_kw(z, cs, trie)).cpu()
        assert torch.equal(ours[:, :skip], seq[:, :skip])
        lg2 = _teacher_forced_logits(m, pix, src, ours, 1)
        live2 = np.cumsum(np.cumsum(ours[:, skip:].numpy() == EOS, 1), 1) <= 1
        for i in range(ours.shape[1] - skip):
            _, got = _step_kept(lg2, ours, skip - 1 + i, kw, ref, which, skip, t_, k_)
            inside = got.gather(1, ours[:, skip + i:skip + i + 1]).squeeze(1)
            assert inside[torch.from_numpy(live2[:, i])].all(), (cs["id"], i)
    assert boundary <= len(cases) // 10, boundary


# ---- cross-checks that need no golden ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(kind):
    """(model, pixels, source ids, max_length): tiny_b in fp32, or the configs[1] shapes in bf16 at B = 64, V = 32128"""
    if kind == "tiny":
        m, g = _build("tiny_b", "fp32", _eos_row("tiny_b"))
        return m, g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda(), 12
    return _configs1_model() + (20,)


KINDS = ["tiny", "configs1"]


def _body(row, skip=1):
    body = row[skip:]
    return body[:body.index(EOS)] if EOS in body else body


def _distinct_phrases(rng, n, V, lengths=(1, 5)):
    """phrases of distinct tokens >= 2 each (no n-gram can repeat inside one), many sharing prefixes"""
    out, seen = [], set()
    while len(out) < n:
        pre = list(rng.choice(out))[:rng.randint(0, 2)] if out and rng.random() < 0.6 else []
        more = max(0, rng.randint(lengths[0], lengths[1]) - len(pre))  # 0: a phrase that is a prefix of another
        p = pre + [t for t in rng.sample(range(2, V), 2 * lengths[1]) if t not in pre][:more]
        if p and tuple(p) not in seen:
            seen.add(tuple(p))
            out.append(p)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_trie_of_the_greedy_outputs_reproduces_them(kind):
    m, pix, src, Lm = _model(kind)
    V = m.main_cfg.vocab_size
    plain, info = m.generate(pix, src, max_length=Lm, return_logprobs=True)
    rng = random.Random(1)
    phrases = [_body(r) for r in plain.tolist()] + _distinct_phrases(rng, 1000, V)
    trie = _trie([phrases], V)
    got, ginfo = m.generate(pix, src, max_length=Lm, return_logprobs=True, constraint=trie)
    assert torch.equal(got, plain)
    assert torch.equal(ginfo["lengths"], info["lengths"])
    # a softmax over fewer tokens: every chosen token is at least as likely
    assert (ginfo["token_logprobs"] >= info["token_logprobs"]).all()
    assert (ginfo["token_logprobs"] > info["token_logprobs"]).any()


@pytest.mark.parametrize("kind", KINDS)
def test_every_returned_row_is_a_phrase_of_its_set(kind):
    m, pix, src, Lm = _model(kind)
    V, B = m.main_cfg.vocab_size, src.shape[0]
    rng = random.Random(2)
    sets = [_distinct_phrases(rng, 300, V), _distinct_phrases(rng, 20, V)]
    trie = _trie(sets, V)
    which = [b % 2 for b in range(B)]
    prompt = torch.tensor([[rng.randrange(2, V), rng.randrange(2, V)] for _ in range(B)], dtype=torch.int64)
    runs = [(dict(), 1), (dict(num_beams=4), 1), (dict(do_sample=True), 1), (dict(no_repeat_ngram_size=2), 1),
            (dict(num_beams=4, no_repeat_ngram_size=2), 1), (dict(do_sample=True, best_of=4, no_repeat_ngram_size=2), 1),
            (dict(decoder_input_ids=prompt), 3), (dict(do_sample=True, top_k=0, decoder_input_ids=prompt), 3)]
    seen = set()
    for kw, skip in runs:
        torch.manual_seed(0)
        out = m.generate(pix, src, max_length=Lm, constraint=trie, constraint_set=which, **kw).cpu()
        assert out.shape[0] == B, kw
        if skip > 1:
            assert torch.equal(out[:, 1:skip], prompt)
        for b, row in enumerate(out.tolist()):
            assert EOS in row[skip:], (kw, row)
            assert trie.contains(_body(row, skip), set=which[b]), (kw, b, row)
            seen.add((which[b], tuple(_body(row, skip))))
    assert len(seen) > 2


@pytest.mark.parametrize("kind", KINDS)
def test_beam_search_over_twelve_phrases_is_exhaustive(kind):
    m, pix, src, Lm = _model(kind)
    V, B = m.main_cfg.vocab_size, src.shape[0]
    rng = random.Random(3)
    a, b, c = rng.sample(range(2, V), 3)
    tails = rng.sample(range(2, V), 12)
    phrases = [[a, b, tails[0]], [a, b, tails[1]], [a, b, tails[2]], [a, c, tails[3]], [a, tails[4], tails[5]], [b, a, tails[6]],
               [b, a, tails[7]], [b, c, tails[8]], [c, tails[9], a], [c, tails[9], b], [c, tails[10], a], [tails[11], a, b]]
    trie = _trie([phrases], V)
    cand = torch.tensor([p + [EOS] for p in phrases], dtype=torch.int64).unsqueeze(0).repeat(B, 1, 1).cuda()
    # max_length = the phrases' length + EOS + the start token: both calls then prefill the same decoder shape and every step runs
    # the same kernels over the same 12 B rows (in bf16 the logits of two prefills of different lengths differ by bf16 roundings,
    # measured up to 7e-3 in a score -- more than the gap below)
    Lm = 5
    for lp in (1.0, 2.0):
        want = m.score(pix, src, cand, length_penalty=lp)
        seq, sc = m.generate(pix, src, max_length=Lm, num_beams=12, num_return_sequences=12, return_scores=True, length_penalty=lp,
                             constraint=trie)
        assert seq.shape[0] == B * 12
        got_idx = torch.tensor([phrases.index(_body(r)) for r in seq.tolist()]).view(B, 12)
        assert (got_idx.sort(1)[0] == torch.arange(12)).all()  # every phrase, once
        ws = want["scores"].cpu()
        sc = sc.cpu().view(B, 12)
        if kind == "tiny":
            assert torch.equal(got_idx, want["order"].cpu()), lp
            assert torch.allclose(sc, ws.gather(1, got_idx), atol=1e-4, rtol=0), lp
        else:  # bf16: the order agrees wherever score()'s gap exceeds 1e-3
            by = ws.gather(1, got_idx)
            assert (by[:, :-1] >= by[:, 1:] - 1e-3).all(), lp


@pytest.mark.parametrize("kind", KINDS)
def test_one_token_phrases_renormalise_over_the_allowed_set(kind):
    m, pix, src, Lm = _model(kind)
    V = m.main_cfg.vocab_size
    toks = sorted(random.Random(4).sample(range(2, V), 9))
    trie = _trie([[[t] for t in toks]], V)
    seq, info = m.generate(pix, src, max_length=Lm, return_logprobs=True, constraint=trie)
    assert seq.shape[1] == 3 and (seq[:, 2] == EOS).all()
    lg = _teacher_forced_logits(m, pix, src, seq.cpu(), 1)[:, 0].float()
    sub = torch.log_softmax(lg[:, toks], -1)
    # fp32: the two forwards run the same kernels over position 0, the log_softmax differs by rounding only.  bf16: a logit of
    # the two forwards (different decoder lengths, different GEMM shapes) may differ by one bf16 ulp at the largest magnitude,
    # 2^(floor(log2 max|x|) - 7), and a log_softmax moves by at most twice the largest change of an entry
    tol = 1e-5 if kind == "tiny" else 2 * 2.0 ** (math.floor(math.log2(float(lg[:, toks].abs().max()))) - 7)
    lp = info["token_logprobs"]
    top2 = torch.topk(sub, 2, -1)[0].cpu()
    clear = (top2[:, 0] - top2[:, 1]) > 2 * tol  # (the pick is the teacher-forced arg-max wherever rounding cannot swap the two)
    assert clear.any() and torch.equal(seq[:, 1].cpu()[clear], torch.tensor(toks)[sub.argmax(-1).cpu()][clear])
    assert torch.allclose(lp[:, 1], sub.max(-1)[0].to(lp.device), atol=tol, rtol=0)
    assert (lp[:, 2] == 0).all() and (info["lengths"] == 2).all()  # EOS alone is allowed: probability 1


def test_nodes_buffer_is_the_host_walk():
    m, pix, src, Lm = _model("tiny")
    V, B = m.main_cfg.vocab_size, src.shape[0]
    rng = random.Random(5)
    sets = [_distinct_phrases(rng, 50, V), _distinct_phrases(rng, 5, V)]
    trie = _trie(sets, V)
    tab = _tables(trie)
    which = [b % 2 for b in range(B)]
    prompt = torch.tensor([[7, 9]] * B, dtype=torch.int64)
    m.generate(pix, src, max_length=Lm, constraint=trie)  # (binds the engine the calls below reuse)
    eng = m._engine
    held = {}
    begin = eng.gen_begin

    def capture(cfg, ws):
        held["ws"] = ws
        return begin(cfg, ws)
    eng.gen_begin = capture
    try:
        for kw, skip, n in ((dict(), 1, 1), (dict(do_sample=True, num_return_sequences=3), 1, 3), (dict(decoder_input_ids=prompt), 3, 1)):
            out = m.generate(pix, src, max_length=Lm, constraint=trie, constraint_set=which, **kw).cpu()
            assert m._engine is eng
            nodes = eng.gen_buffer(held["ws"], "nodes").cpu()
            assert nodes.dtype == torch.int32 and nodes.shape == (B * n, 1)
            # the node every row stood on when its last position was chosen: the walk over the tokens chosen before it
            want = [walk(tab, row[skip:-1], which[r // n]) for r, row in enumerate(out.tolist())]
            assert nodes.flatten().tolist() == want, kw
    finally:
        del eng.gen_begin
    m.generate(pix, src, max_length=Lm)  # a session without a constraint has no such buffer
    with pytest.raises(KeyError):
        eng.gen_buffer(held["ws"], "nodes")


def test_sessions_without_a_constraint_are_unchanged():
    m, pix, src, Lm = _model("tiny")
    V, B = m.main_cfg.vocab_size, src.shape[0]
    trie = _trie([[[5], [6, 7]]], V)
    roots = trie.roots[torch.zeros(B, dtype=torch.int64, device="cuda")].contiguous()
    m.generate(pix, src, max_length=Lm)
    eng = m._engine
    for mode, n, procs in (("pick", 1, None), ("sample", 3, None), ("beam", 4, None),
                           ("beam", 4, dict(repetition_penalty=1.2, no_repeat_ngram_size=0, bad_words_ids=[], min_length=0, min_new_tokens=0))):
        plain = eng.gen_cfg(mode, n, Lm, EOS, 0, procs=procs)
        zeroed = eng.gen_cfg(mode, n, Lm, EOS, 0, procs=procs, constraint=(trie, roots))
        with_bytes = eng.gen_workspace_bytes(zeroed)
        zeroed.constraint = None  # (asking for the size above left nothing armed)
        assert eng.gen_workspace_bytes(plain) == eng.gen_workspace_bytes(zeroed) > 0
        grow = with_bytes - eng.gen_workspace_bytes(plain)
        rows_bytes = 0 if procs is not None else B * n * V * 4
        assert 2 * B * n * 4 + rows_bytes <= grow <= 2 * B * n * 4 + rows_bytes + 3 * 256, (mode, grow)
    bad = eng.gen_cfg("force", 2, Lm, EOS, 0, want_logprobs=True, constraint=(trie, roots))
    assert eng.gen_workspace_bytes(bad) == 0
    for kw in (dict(), dict(num_beams=4), dict(do_sample=True, temperature=1.3, top_k=0)):
        torch.manual_seed(7)
        a = m.generate(pix, src, max_length=Lm, **kw)
        torch.manual_seed(7)
        b = m.generate(pix, src, max_length=Lm, constraint=None, constraint_set=None, **kw)
        m.generate(pix, src, max_length=Lm, constraint=trie, **kw)  # a constrained session in between leaves nothing behind
        torch.manual_seed(7)
        c = m.generate(pix, src, max_length=Lm, **kw)
        assert torch.equal(a, b) and torch.equal(a, c), kw
