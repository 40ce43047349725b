"""Several captions per image through MyModel: labels [B, n, Lt] over B images, one pass of the Swin tower and both encoders per image.

Model and weights are golden tiny_b's (two Swin stages with 49 image tokens, three decoder layers, head dim 32, vocabulary 512),
the images and source ids its two different samples (Ls = 20, so Le = 69: the cross-attention's keys pass one 64-key block); the
captions are drawn here, different everywhere, so that b / n mistaken for b % n, or a caption attached to the wrong image, changes
the loss and every gradient.  The reference is the CPU oracle on the repeat-interleaved batch -- pixel_values and source ids
repeat_interleave(n, 0), labels viewed [B*n, Lt] -- computed once per set of labels and shared.

Yardsticks are those tests/test_model_gpu.py applies to the ungrouped step against the oracle: fp32 engine loss rel <= 2e-5 and
rel-L2 <= 1e-4 on every gradient tensor; bf16 engine loss rel <= 2e-3 and gradient cosine >= 0.99.  token_losses() is held to the
loss tolerance as a vector (rel-L2).

"Bit for bit" between two runs follows the project's rule for float atomics (tests/test_loss_opts_gpu.py): the tied table's
scatter-add and the two relative-position tables are written with float atomics and do not repeat their bits between two plain runs
of the SAME model (with the trainable tower neither do the Swin gradients: these tests keep it frozen), so for those three, and
only for them, the distance to the other run stays within twice the spread of three reference runs (floor 2^-22 of the norm).
The loss, the per-token losses and every other gradient tensor must have the same bits, and the reference runs must repeat their
own bits there: a tensor that does not is a failure, not an exception made at run time."""
import functools
import types

import pytest
import torch

from tests.helpers import cosine, load_golden, rel_l2

pytestmark = pytest.mark.gpu

CASES = [(3, 5), (5, 17), (2, 32)]  # (n, Lt): n*Lt = 15 inside one query tile, 85 across the 64-query tile, 64 exactly one
ATOMIC = ("shared.weight", "relative_attention_bias.weight")
LOSS_TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-3}


def build(dtype=torch.float32, train_swin=False, train=False):
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_golden("tiny_b")
    sw, t5 = SwinConfig.from_dict(g["meta"]["swin_config"]), T5Config.from_dict(g["meta"]["t5_config"])
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=train_swin,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], g["sds"]["main"]), dtype=dtype).to("cuda")
    m._direct_grads = True
    m.transformer.train(train)
    return m


@functools.lru_cache(maxsize=None)
def labels(n, Lt, variant="full"):
    """int64 [2, n, Lt] on the host: every caption different, closed by EOS, one with two scored pads behind its EOS; variant
    'pad': caption 1 of image 0 is all -100 (an image with fewer captions).  Shared: never written."""
    V = load_golden("tiny_b")["t5_cfg"].vocab_size
    t = torch.randint(2, V, (2, n, Lt), generator=torch.Generator().manual_seed(100 * n + Lt))
    t[..., -1] = 1
    t[1, n - 1, -3] = 1
    t[1, n - 1, -2:] = 0
    if variant == "pad":
        t[0, 1] = -100
    assert len({tuple(r.tolist()) for r in t.view(-1, Lt)}) == 2 * n
    return t


def inputs():
    inp = load_golden("tiny_b")["inputs"]
    assert not torch.equal(inp["pixel_values"][0], inp["pixel_values"][1]) and not torch.equal(inp["src_ids"][0], inp["src_ids"][1])
    return inp["pixel_values"], inp["src_ids"]


@functools.lru_cache(maxsize=None)
def oracle(n, Lt, variant="full"):
    """(loss, token losses [2, n, Lt], {main grads}, {swin grads}) of the oracle on the repeat-interleaved batch; never written"""
    from oracle import swin_t5_oracle as O
    g = load_golden("tiny_b")
    pix, src = inputs()
    tgt = labels(n, Lt, variant).view(2 * n, Lt)
    main = {k: v.clone().requires_grad_(True) for k, v in g["sds"]["main"].items()}
    swin = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in g["sds"]["swin"].items()}
    loss, parts = O.mymodel_forward(swin, g["sds"]["lang"], main, g["swin_cfg"], g["t5_cfg"], g["t5_cfg"], pix.repeat_interleave(n, 0),
                                    src.repeat_interleave(n, 0), tgt, training=False, image_model_train=True, return_parts=True)
    loss.backward()
    tl = torch.nn.functional.cross_entropy(parts["logits"].detach().view(2 * n * Lt, -1), tgt.reshape(-1), ignore_index=-100,
                                           reduction="none").view(2, n, Lt)
    grab = lambda sd: {k: v.grad.detach() for k, v in sd.items() if torch.is_tensor(v) and v.requires_grad and v.grad is not None}
    return float(loss.detach()), tl, grab(main), grab(swin)


def step(m, tgt, weights=None, backward=True):
    pix, src = inputs()
    te = {"input_ids": tgt.cuda()}
    if weights is not None:
        te["loss_weights"] = weights.cuda()
    loss = m({"pixel_values": pix.cuda()}, {"input_ids": src.cuda()}, te)
    if backward:
        loss.backward()
    assert int(m._engine.err_view.item()) == 0
    return loss.detach()


def native_grads(m):
    out = {("main", k): p.grad.detach().clone() for k, p in m.transformer.named_parameters() if p.grad is not None}
    out.update({("swin", k): p.grad.detach().clone() for k, p in m.image_model.named_parameters() if p.grad is not None})
    return out


def against_oracle(m, loss, n, Lt, variant, dtype, train_swin):
    want_loss, want_tl, gmain, gswin = oracle(n, Lt, variant)
    tol = LOSS_TOL[dtype]
    tl = m.token_losses()
    got = native_grads(m)
    print(f"n={n} Lt={Lt} {variant} {dtype} train_swin={train_swin}: loss {float(loss)} oracle {want_loss}, "
          f"token losses rel-L2 {rel_l2(tl.cpu(), want_tl):.3e}")
    assert tuple(tl.shape) == (2, n, Lt)
    assert abs(float(loss) - want_loss) <= tol * abs(want_loss), (float(loss), want_loss)
    assert rel_l2(tl.cpu(), want_tl) <= tol
    assert bool((tl.cpu()[labels(n, Lt, variant) == -100] == 0).all())
    wants = {("main", k): v for k, v in gmain.items()}
    if train_swin:
        wants.update({("swin", k): v for k, v in gswin.items()})
    else:
        assert not any(k[0] == "swin" for k in got)
    assert set(got) == set(wants), set(got) ^ set(wants)
    worst, a, b = (0.0, None), [], []
    for k, ref in wants.items():
        a.append(got[k].cpu().flatten())
        b.append(ref.flatten())
        if float(ref.abs().max()) == 0.0:
            assert dtype != torch.float32 or float(got[k].abs().max()) < 1e-10, k
            continue
        e = rel_l2(got[k].cpu(), ref)
        worst = max(worst, (e, k))
        if dtype == torch.float32:
            assert e <= 1e-4, (k, e)
    c = cosine(torch.cat(a), torch.cat(b))
    print(f"    worst gradient rel-L2 {worst}, overall cosine {c}")
    assert c >= (0.99999 if dtype == torch.float32 else 0.99), c


# ---- 1. against the oracle, dropout off -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,Lt", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_grouped_step_matches_the_oracle_on_the_repeated_batch(dtype, n, Lt):
    """the trainable tower: every T5 gradient and every Swin gradient"""
    m = build(dtype, train_swin=True)
    loss = step(m, labels(n, Lt))
    assert loss.dim() == 0 and loss.dtype == torch.float32
    against_oracle(m, loss, n, Lt, "full", dtype, True)


def test_grouped_step_with_the_frozen_tower():
    n, Lt = CASES[0]
    m = build(torch.float32, train_swin=False)
    against_oracle(m, step(m, labels(n, Lt)), n, Lt, "full", torch.float32, False)


STREAMING = (11, 30)  # n*Lt = 330 queries over Le = 69 keys at head dim 32


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_grouped_step_past_the_one_workgroup_attention_backward(dtype):
    """the kernels of the headline grouped shapes (n = 5, Lt = 64: 320 queries, 58 keys, head dim 64): with n*Lt this long the
    bf16 cross-attention forward is the matrix-core kernel over several query tiles and its backward no longer fits one
    workgroup's LDS, so klab_t5_attn_bwd runs the streaming d q and d k / d v kernels (the fp32 engine: the generic kernels over
    21 query tiles).  Lt stays below 64, as there: the decoder's self-attention keeps its fused kernels."""
    from tests import exact_ref as R
    n, Lt = STREAMING
    Le = 49 + inputs()[1].shape[1]
    assert Le == 69 and not R.mfma_bwd_fits(n * Lt, Le, 32) and all(R.mfma_bwd_fits(a * b, Le, 32) for a, b in CASES)
    m = build(dtype, train_swin=True)
    against_oracle(m, step(m, labels(n, Lt)), n, Lt, "full", dtype, True)


def test_generate_and_score_after_a_grouped_step_bind_ungrouped():
    """they bind with n = 1: the same tokens and scores as on a model that never saw a grouped batch"""
    n, Lt = CASES[0]
    pix, src = inputs()
    cand = labels(n, Lt)
    outs = []
    for grouped_first in (False, True):
        m = build()
        if grouped_first:
            step(m, labels(n, Lt))
            m.zero_grad(set_to_none=True)
        seq = m.generate(pix.cuda(), src.cuda(), max_length=8)
        sc = m.score(pix.cuda(), src.cuda(), cand.cuda())
        outs.append((seq.cpu(), sc["token_logprobs"].cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert tuple(outs[0][1].shape) == (2, n, Lt) and m._bound_key[-1] == 1


# ---- 2. exactness of the surface --------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_values(a, b):
    """equal as numbers: same_bits but for the sign of a zero"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def assert_same_run(what, got, refs, equal=same_bits, token_losses=True):
    """got / refs[i]: dict(loss, tl, grads), at least two reference runs.  As tests/test_loss_opts_gpu.py: the reference runs repeat
    their own bits in the loss, the per-token losses and every gradient tensor but the three of ATOMIC, and `got` is `equal` to
    them there; the three of ATOMIC stay within twice the spread of the reference runs (module docstring)."""
    ref = refs[0]
    assert len(refs) >= 2
    assert set(got["grads"]) == set(ref["grads"])
    for q in refs[1:]:  # the yardstick repeats itself
        assert same_bits(q["loss"].cpu(), ref["loss"].cpu()) and same_bits(q["tl"].cpu(), ref["tl"].cpu()), what
    wander = [k for k, r in ref["grads"].items() if not k[1].endswith(ATOMIC) and not all(same_bits(q["grads"][k], r) for q in refs[1:])]
    print(f"{what}: {len(ref['grads'])} gradient tensors; the reference runs do not repeat the bits of {wander} (ATOMIC apart)")
    assert not wander, (what, wander)
    assert same_bits(got["loss"].cpu(), ref["loss"].cpu()), (what, float(got["loss"]), float(ref["loss"]))
    if token_losses:
        assert same_bits(got["tl"].cpu(), ref["tl"].cpu()), what
    dist = lambda a, b: float((a.double() - b.double()).norm())
    pairs = [(i, j) for i in range(len(refs)) for j in range(i + 1, len(refs))]
    differ = []
    for k, r in ref["grads"].items():
        if k[1].endswith(ATOMIC):
            spread = max(dist(refs[i]["grads"][k], refs[j]["grads"][k]) for i, j in pairs)
            allowed = max(2.0 * spread, 2.0 ** -22 * float(r.double().norm()))
            print(f"    {k[1]}: distance to a reference run {dist(got['grads'][k], r):.3e}, between reference runs {spread:.3e}")
            assert dist(got["grads"][k], r) <= allowed, (what, k, dist(got["grads"][k], r), spread)
        elif not equal(got["grads"][k], r):
            differ.append((k, dist(got["grads"][k], r)))
    assert not differ, (what, differ)


def record(m, loss):
    return dict(loss=loss.clone(), tl=m.token_losses(), grads=native_grads(m))


@functools.lru_cache(maxsize=None)
def fresh_runs(n, Lt, three_d, copies=3):
    """eval-mode steps of `copies` fresh fp32 models (frozen tower) on the same labels: labels(n, Lt) as [2, n, Lt] when three_d,
    else (n = 1) the same ids as [2, Lt]"""
    out = []
    for _ in range(copies):
        m = build()
        tgt = labels(n, Lt) if three_d else labels(1, Lt).view(2, Lt)
        out.append(record(m, step(m, tgt)))
    return tuple(out)


def test_three_d_with_one_caption_is_the_two_d_call_bit_for_bit():
    Lt = 17
    two_d = fresh_runs(1, Lt, False)
    m = build()
    got = record(m, step(m, labels(1, Lt)))
    assert tuple(got["tl"].shape) == (2, 1, Lt) and tuple(two_d[0]["tl"].shape) == (2, Lt)
    got["tl"] = got["tl"].view(2, Lt)
    assert_same_run("[B, 1, Lt] against [B, Lt]", got, two_d)
    assert m._bound_key == (2, 20, Lt, torch.device("cuda", torch.cuda.current_device()), 1)


def test_rebinding_between_grouped_and_ungrouped_batches():
    """a 2-D call after a grouped call, and the reverse, each equal to its own fresh-model result"""
    n, Lt = 5, 17
    two_d, grouped = fresh_runs(1, Lt, False), fresh_runs(n, Lt, True)
    m = build()
    step(m, labels(n, Lt))
    m.zero_grad(set_to_none=True)
    key_grouped = m._bound_key
    eng = m._engine  # the grouped bind took the caption count with it: what a plain klab_engine_bind would make now is ungrouped
    assert eng.captions == n
    assert int(eng._lib.klab_engine_workspace_bytes(eng._h, 2, 20, Lt)) == eng.workspace_bytes(2, 20, Lt) < eng.workspace_bytes(2, 20, Lt, n)
    assert_same_run("2-D after grouped", record(m, step(m, labels(1, Lt).view(2, Lt))), two_d)
    assert m._bound_key != key_grouped and m._bound_key[-1] == 1 and key_grouped[-1] == n
    m.zero_grad(set_to_none=True)
    assert_same_run("grouped after 2-D", record(m, step(m, labels(n, Lt))), grouped)
    assert m._bound_key == key_grouped


def test_two_grouped_training_steps_with_the_same_seed_repeat():
    n, Lt = 5, 17
    runs = []
    for _ in range(4):
        torch.manual_seed(4321)
        m = build(train=True)
        first = record(m, step(m, labels(n, Lt)))
        m.zero_grad(set_to_none=True)
        second = record(m, step(m, labels(n, Lt)))
        runs.append((first, second))
    eval_loss = oracle(n, Lt)[0]
    assert float(runs[0][0]["loss"]) != float(runs[0][1]["loss"])  # the mask stream advances ...
    assert abs(float(runs[0][0]["loss"]) - eval_loss) > 1e-4 * eval_loss  # ... and is on
    for i in (0, 1):
        assert_same_run(f"grouped training step {i}", runs[3][i], [runs[0][i], runs[1][i], runs[2][i]])


# ---- 3. padding captions ----------------------------------------------------------------------------------------------------------
def test_a_caption_of_minus_100_adds_nothing():
    n, Lt = CASES[0]
    m = build(train_swin=True)
    loss = step(m, labels(n, Lt, "pad"))
    against_oracle(m, loss, n, Lt, "pad", torch.float32, True)
    tl = m.token_losses().cpu()
    assert bool((tl[0, 1] == 0).all()) and bool((tl[0, 0] != 0).all()) and bool((tl[1] != 0).all())
    assert abs(float(loss) - oracle(n, Lt)[0]) > 1e-4 * abs(float(loss))  # (the caption did count before)


def test_a_zero_weight_caption_is_the_minus_100_form():
    """weights of 1 with one caption at 0 on the full labels: sum w l / sum w has the terms and the divisor of the -100 form's mean
    (the rows of a caption never meet another caption's in the decoder), so loss and every gradient are the -100 form's within the
    fp32 engine's own yardsticks -- the two forms run different cross-entropy kernels -- and therefore the oracle's on those labels"""
    n, Lt = CASES[0]
    m = build(train_swin=True)
    w = torch.ones(2, n, Lt)
    w[0, 1] = 0
    loss = step(m, labels(n, Lt), weights=w)
    ref = build(train_swin=True)
    ref_loss = step(ref, labels(n, Lt, "pad"))
    assert abs(float(loss) - float(ref_loss)) <= 2e-5 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    got, want = native_grads(m), native_grads(ref)
    assert set(got) == set(want)
    same = 0
    for k, r in want.items():
        if float(r.abs().max()) == 0.0:
            assert float(got[k].abs().max()) < 1e-10, k
            continue
        assert rel_l2(got[k].cpu(), r.cpu()) <= 1e-4, (k, rel_l2(got[k].cpu(), r.cpu()))
        same += same_bits(got[k], r)
    print(f"zero-weight caption against -100 caption: {same} of {len(want)} gradient tensors have the same bits")
    # token_losses are unweighted: the caption's row is there, and the weighted mean leaves it out
    tl = m.token_losses().cpu().double()
    assert bool((tl[0, 1] != 0).all())
    assert abs(float((w.double() * tl).sum() / w.sum()) - float(loss)) <= 1e-6 * abs(float(loss))
    against_oracle_grads = oracle(n, Lt, "pad")[2]
    for k, r in against_oracle_grads.items():
        if float(r.abs().max()) > 0.0:
            assert rel_l2(got[("main", k)].cpu(), r) <= 1e-4, k


def test_a_zero_weight_caption_equals_the_minus_100_caption_under_unit_weights():
    """the same cross-entropy kernel on both sides: full labels with weights 1 but for one caption at 0, against that caption at
    -100 with weights all 1 (frozen tower, three fresh reference runs).  Row by row the kernel computes the same numbers: a row
    counts w into the divisor and w l into the loss, 0 for a zero weight as for a label of -100, and d logits of such a row are
    g (...) with g = w / W = 0 -- zeros in both forms, of which the zero-weight form's element at the label is (p - 1) 0 = -0.
    A zero of either sign adds nothing to any sum behind it, so the loss has the -100 form's bits and every gradient its values
    (same_values: the sign of a zero apart); the three tensors float atomics write follow the rule for atomics."""
    n, Lt = CASES[0]
    ones = torch.ones(2, n, Lt)
    refs = []
    for _ in range(3):
        r = build()
        refs.append(record(r, step(r, labels(n, Lt, "pad"), weights=ones)))
    w = ones.clone()
    w[0, 1] = 0
    m = build()
    got = record(m, step(m, labels(n, Lt), weights=w))
    # (token_losses are unweighted: the zero-weight caption's row is there, the -100 caption's is zero -- not compared)
    assert_same_run("zero-weight caption against -100 caption, unit weights", got, refs, equal=same_values, token_losses=False)
    keep = torch.ones(2, n, Lt, dtype=torch.bool)
    keep[0, 1] = False
    assert same_bits(got["tl"].cpu()[keep], refs[0]["tl"].cpu()[keep]) and bool((refs[0]["tl"].cpu()[0, 1] == 0).all())
    assert any(float(v.abs().max()) > 0 for v in got["grads"].values())


def test_a_wrong_weights_shape_is_refused_by_name():
    n, Lt = CASES[0]
    m = build()
    plain = float(step(m, labels(n, Lt), backward=False))
    for bad in (torch.ones(2, Lt), torch.ones(2 * n, Lt), torch.ones(2, n, Lt + 1), torch.ones(2, n, Lt, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"\[B, n, Lt\]"):
            step(m, labels(n, Lt), weights=bad, backward=False)
        assert float(step(m, labels(n, Lt), backward=False)) == plain  # nothing stayed armed
    with pytest.raises(ValueError, match=r"\[B, n, Lt\] is on cpu"):
        pix, src = inputs()
        m({"pixel_values": pix.cuda()}, {"input_ids": src.cuda()}, {"input_ids": labels(n, Lt).cuda(), "loss_weights": torch.ones(2, n, Lt)})


# ---- 5. optimizer plumbing --------------------------------------------------------------------------------------------------------
def test_grouped_step_keeps_the_fused_optimizer_clip_and_ema():
    from klab_multimodalmodel_amd import optim
    n, Lt = CASES[1]
    m = build(train=True)
    opt = optim.FusedAdamW(m.transformer.parameters(), lr=1e-3, step_in_backward=True)
    ema = optim.WeightEMA(m, decay=0.9)
    before = [p.detach().clone() for p in m.transformer.parameters()]
    for i in range(2):
        step(m, labels(n, Lt))
        if i == 0:  # (once segment 0 is updated underneath the backward the whole-gradient clip is refused: test_grad_clip_gpu.py)
            params = [p for p in m.transformer.parameters() if p.grad is not None]
            st, owner = optim._clip_native(params, [p.grad for p in params], 2.0)
            assert st is not None and owner is m, owner
            want = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad.double()) for p in params]))
            total = optim.clip_grad_norm_(m.transformer.parameters(), 0.5 * float(want))
            assert abs(float(total) - float(want)) <= 1e-6 * float(want)
            names, norms = m.grad_norms()
            assert len(names) + 1 == norms.numel() and bool(torch.isfinite(norms).all())
        opt.step()
        opt.zero_grad()
        ema.update()
        assert opt._fallback is None and opt._fb_reason is None, opt._fb_reason
        assert ema._fb_reason is None and ema._flat is not None, ema._fb_reason
    assert opt.in_backward_updates == 1 and ema.num_updates == 2
    assert m.flat_grads("main") is not None and m._bound_key[-1] == n
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, m.transformer.parameters()))
    torch.cuda.synchronize()


def test_grouped_step_under_graph_replay():
    """eager, captured, replayed with fresh input tensors, then other labels through the same graph, grouped and ungrouped side by
    side: the grouped replay equals its eager step in the bits of everything whose bits the ungrouped replay keeps (printed), and
    within the fp32 engine's gradient yardstick (rel-L2 <= 1e-4) everywhere"""
    n, Lt = 5, 17
    res = {}
    for grouped in (False, True):
        for graph in (False, True):
            m = build()
            m.use_graph = graph
            out = []
            for s in range(4):
                tgt = labels(n, Lt) if grouped else labels(1, Lt).view(2, Lt)
                if s == 3:
                    tgt = tgt.flip(-1).contiguous()
                out.append(record(m, step(m, tgt.clone())))
                m.zero_grad(set_to_none=True)
            res[grouped, graph] = out
            del m
    keeps = None  # what the ungrouped replay keeps bit for bit at every step
    for grouped in (False, True):
        equal = {"loss": True, "tl": True}
        for e, r in zip(res[grouped, False], res[grouped, True]):
            assert abs(float(e["loss"]) - float(r["loss"])) <= 1e-6 * abs(float(e["loss"]))
            equal["loss"] &= same_bits(e["loss"], r["loss"])
            equal["tl"] &= same_bits(e["tl"], r["tl"])
            for k, v in e["grads"].items():
                assert rel_l2(r["grads"][k].cpu(), v.cpu()) <= 1e-4, (grouped, k)
                equal[k] = equal.get(k, True) and same_bits(v, r["grads"][k])
        print("grouped" if grouped else "ungrouped", "replay keeps the eager bits of", sum(equal.values()), "of", len(equal), "results;",
              "not of", sorted(str(k) for k, v in equal.items() if not v))
        if not grouped:
            keeps = {k for k, v in equal.items() if v and not (isinstance(k, tuple) and k[1].endswith(ATOMIC))}
            assert "loss" in keeps and "tl" in keeps
        else:
            lost = sorted(str(k) for k in keeps if not equal[k])
            assert not lost, lost
    g = res[True, True]
    assert same_bits(g[0]["loss"], g[1]["loss"]) and same_bits(g[1]["loss"], g[2]["loss"]) and abs(float(g[3]["loss"]) - float(g[0]["loss"])) > 1e-3
