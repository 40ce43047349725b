"""T5 v1.1 / Flan-T5 support on the GPU: the gate kernels through the C ABI against an fp32 restatement, the whole model against
the reference's own outputs (tests/golden/tiny_v11_*), generation, FusedAdam, checkpoint resume and a t5-v1_1-small sized run.

Bounds are the project's: tests/test_ops_gpu.py::tol per kernel (relative L2 2e-5 fp32, 1.5e-2 bf16); the fp32 engine's loss <= 1e-5,
activations <= 2e-5, gradients <= 1e-4 (test_fp32_engine_matches_reference); bf16: loss 2e-3, cosine 0.99 overall / 0.97 per tensor
and relative L2 <= 2 x the reference's own bf16 error stored in the fixture (per tensor with the overall error as the floor)."""
import math
import os

import pytest
import torch

from tests.helpers import cosine, rel_l2
from tests.logits_proc_ref import hf_process
from tests.sample_ref import boundary_tokens, hf_warp
from tests.v11_helpers import NAMES, args, build_v11, geglu_bwd_ref, geglu_ref, load_v11, run

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16]


def tol(dt):  # tests/test_ops_gpu.py::tol
    return 2e-5 if dt == torch.float32 else 1.5e-2


def _gate_inputs(M, F, dt, seed=0):
    g = torch.Generator().manual_seed(seed + M + F)
    ab = (torch.randn(M, 2 * F, generator=g) * 1.5).to(dt)
    # gelu_new(a) * b is never exactly zero: 0.05 <= |a| <= 4 keeps gelu_new(a) away from 0 on both sides (tanh rounds to -1, and
    # gelu_new to an exact 0, from a = -5.5 down in fp32), and |b| >= 0.05
    ab = torch.where(ab.float().abs() < 0.05, torch.full_like(ab, 0.0625), ab).clamp(-4.0, 4.0)
    dh = torch.randn(M, F, generator=g).to(dt)
    return ab.cuda(), dh.cuda()


# ---------------------------------------------------------------------------------------------------------------- gate kernels
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,F", [(21, 320), (130, 1024), (77, 2816), (576, 1024), (3, 64)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_geglu_kernels_match_restatement(dt, M, F, p):
    from klab_multimodalmodel_amd import ops as K
    ab, dh = _gate_inputs(M, F, dt)
    sd = torch.tensor([4321], dtype=torch.int32).cuda()
    h = torch.empty(M, F, dtype=dt, device="cuda")
    K.geglu_fwd(ab, h, drop_p=p, seed_dev=sd, tag=0x20015)
    a, b = ab[:, :F].float(), ab[:, F:].float()
    keep = (h != 0)
    if p == 0.0:
        assert keep.all()
    else:
        assert abs(keep.float().mean().item() - (1 - p)) < 0.02 + 2.0 / math.sqrt(M * F)
    ks = keep.float() / (1 - p)
    e = rel_l2(h.float().cpu(), geglu_ref(a, b, ks).cpu())
    dab = torch.empty(M, 2 * F, dtype=dt, device="cuda")
    K.geglu_bwd(dh, ab, dab, drop_p=p, seed_dev=sd, tag=0x20015)
    da, db = geglu_bwd_ref(dh.float(), a, b, ks)
    ea, eb = rel_l2(dab[:, :F].float().cpu(), da.cpu()), rel_l2(dab[:, F:].float().cpu(), db.cpu())
    print("geglu", dt, M, F, p, "h", e, "da", ea, "db", eb)
    assert e < tol(dt) and ea < tol(dt) and eb < tol(dt), (e, ea, eb)
    assert torch.equal(dab[:, F:] != 0, keep) and torch.equal(dab[:, :F] != 0, keep)  # backward regenerated the forward's mask


def test_geglu_dropout_mask_follows_seed_and_tag():
    from klab_multimodalmodel_amd import ops as K
    M, F, p = 256, 320, 0.1
    ab, _dh = _gate_inputs(M, F, torch.bfloat16)

    def mask(seed, tag):
        h = torch.empty(M, F, dtype=torch.bfloat16, device="cuda")
        K.geglu_fwd(ab, h, drop_p=p, seed_dev=torch.tensor([seed], dtype=torch.int32).cuda(), tag=tag)
        return h != 0

    k0 = mask(77, 5)
    assert torch.equal(mask(77, 5), k0)
    assert not torch.equal(mask(77, 6), k0) and not torch.equal(mask(78, 5), k0)
    # ... and it is the function the GEMM epilogue uses for the same (seed, tag, element index): a ReLU layer and a gated layer of the
    # same shape drop the same elements
    A = torch.full((M, 32), 1.0 / 32).cuda()
    B = torch.ones(F, 32).cuda()
    Cd = torch.empty(M, F, device="cuda")
    K.gemm(A, B, Cd, M=M, N=F, K=32, drop_p=p, seed=torch.tensor([77], dtype=torch.int32).cuda(), tag=5)
    assert torch.equal(Cd != 0, k0)


def test_geglu_strided_rows_and_argument_checks():
    from klab_multimodalmodel_amd import ops as K
    M, F = 37, 192
    ab, dh = _gate_inputs(M, F, torch.float32)
    wide = torch.zeros(M, 2 * F + 64, device="cuda")
    wide[:, :2 * F] = ab
    h = torch.full((M, F + 8), 7.0, device="cuda")
    K.geglu_fwd(wide[:, :2 * F], h[:, :F])
    assert rel_l2(h[:, :F].cpu(), geglu_ref(ab[:, :F], ab[:, F:], torch.ones(M, F, device="cuda")).cpu()) < 2e-5
    assert (h[:, F:] == 7.0).all()  # nothing past the row's F columns was written
    with pytest.raises(NotImplementedError):
        K.geglu_fwd(torch.zeros(4, 2 * 12, device="cuda"), torch.zeros(4, 12, device="cuda"))  # F % 8


# ------------------------------------------------------------------------------------------------------------------ whole model
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("train_swin", [False, True])
def test_fp32_engine_matches_reference_v11(name, train_swin):
    m, g = build_v11(name, torch.float32, train_swin)
    m = m.to("cuda")
    m.transformer.eval()
    loss = run(m, g)
    eng = m._engine
    B = g["inputs"]["src_ids"].shape[0]
    cat = torch.cat([g["acts"]["image_embeddings"], g["acts"]["language_embeddings"]], dim=1)
    d = cat.shape[-1]
    ea = [rel_l2(eng.buffer("encoder_input").float().cpu().view(B, -1, d), cat),
          rel_l2(eng.buffer("encoder_out").float().cpu().view(B, -1, d), g["acts"]["encoder_out"]),
          rel_l2(eng.buffer("decoder_out").float().cpu().view(B, -1, d), g["acts"]["decoder_out"])]
    print(name, train_swin, "loss", loss.item(), "ref", g["loss"], "activations", ea)
    assert max(ea) < 2e-5, ea
    assert abs(loss.item() - g["loss"]) <= 1e-5 * abs(g["loss"])
    loss.backward()
    assert int(eng.err_view.item()) == 0
    assert "lm_head.weight" in g["grads"]["main"] and "shared.weight" in g["grads"]["main"]
    worst = ("", 0.0)
    for mname, tree in (("main", m.transformer), ("swin", m.image_model)):
        for k, ref in g["grads"][mname].items():
            p = tree.get_parameter(k)
            if mname == "swin" and not train_swin:
                assert p.grad is None
                continue
            assert p.grad is not None, k
            if float(ref.abs().max()) == 0.0:
                assert float(p.grad.abs().max()) < 1e-10, k
                continue
            e = rel_l2(p.grad.cpu(), ref)
            worst = max(worst, (k, e), key=lambda t: t[1])
            assert e < 1e-4, (mname, k, e)
    print(name, train_swin, "worst grad", worst)
    assert not torch.equal(m.transformer.get_parameter("lm_head.weight").grad, m.transformer.get_parameter("shared.weight").grad)
    for p in m.language_model.parameters():
        assert p.grad is None


@pytest.mark.parametrize("name", NAMES)
def test_bf16_engine_within_twice_the_references_bf16_error(name):
    m, g = build_v11(name, torch.bfloat16, True)
    m = m.to("cuda")
    m.transformer.eval()
    loss = run(m, g)
    assert abs(loss.item() - g["loss"]) <= 2e-3 * abs(g["loss"]), (loss.item(), g["loss"])
    loss.backward()
    err = g["meta"]["bf16_reference_error"]
    a, b, viol = [], [], []
    for mname, tree in (("main", m.transformer), ("swin", m.image_model)):
        for k, ref in g["grads"][mname].items():
            got = tree.get_parameter(k).grad.cpu()
            if float(ref.norm()) > 1e-6 * ref.numel() ** 0.5:
                c, r = cosine(got, ref), rel_l2(got, ref)
                bound = 2 * max(err[f"g.{mname}.{k}"], err["all"])
                if c <= 0.97 or r > bound:
                    viol.append((mname, k, "cosine", round(c, 4), "rel-L2", round(r, 4), "bound", round(bound, 4)))
            a.append(got.flatten())
            b.append(ref.flatten())
    c, r = cosine(torch.cat(a), torch.cat(b)), rel_l2(torch.cat(a), torch.cat(b))
    print(name, "bf16 loss", loss.item(), "ref", g["loss"], "grad cosine", c, "rel-L2", r, "the reference's own bf16 rel-L2", err["all"])
    assert not viol, viol
    assert c > 0.99 and r <= 2 * err["all"], (c, r, err["all"])


# ------------------------------------------------------------------------------------------------------------------- generation
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kv_cache", [True, False])
def test_generate_greedy_equals_the_references_ids(name, kv_cache):
    m, g = build_v11(name, torch.float32, False)
    m = m.to("cuda")
    pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
    ids = m.generate(pix, src, max_length=g["meta"]["effective"]["generation_max_length"], kv_cache=kv_cache).cpu()
    assert ids.shape == g["greedy_ids"].shape and torch.equal(ids, g["greedy_ids"]), (ids, g["greedy_ids"])  # every position


def _teacher_forced_logits(m, pix, src, seq, n):
    tgt = seq[:, 1:].contiguous().cuda()
    pr, sr = pix.repeat_interleave(n, 0).contiguous(), src.repeat_interleave(n, 0).contiguous()
    eng = m._engine_for(pr, sr, tgt)
    eng.forward(pr, sr, tgt, training=0, seed=0, want_grad=False)
    return eng.buffer("logits").float().view(tgt.shape[0], tgt.shape[1], -1).clone()


@pytest.mark.parametrize("name", NAMES)
def test_generate_beam_sampling_and_processors(name):
    m, g = build_v11(name, torch.float32, False)
    m = m.to("cuda")
    cfg = m.main_cfg
    pix, src = g["inputs"]["pixel_values"].cuda(), g["inputs"]["src_ids"].cuda()
    B, ml = src.shape[0], 12
    greedy = m.generate(pix, src, max_length=ml)
    # sampling with top_k = 1 and beam search with one beam ... are greedy decoding
    assert torch.equal(m.generate(pix, src, max_length=ml, do_sample=True, top_k=1), greedy)
    # beam search: sorted, repeatable, and each score is the teacher-forced sum of log-probabilities / length ** length_penalty
    k = 3
    seq, sc = m.generate(pix, src, max_length=ml, num_beams=k, num_return_sequences=k, return_scores=True)
    seq2, sc2 = m.generate(pix, src, max_length=ml, num_beams=k, num_return_sequences=k, return_scores=True)
    assert torch.equal(seq, seq2) and torch.equal(sc, sc2) and seq.shape[0] == B * k
    assert (sc.view(B, k)[:, :-1] >= sc.view(B, k)[:, 1:]).all()
    logp = torch.log_softmax(_teacher_forced_logits(m, pix, src, seq, k), -1)
    tok = seq[:, 1:].cuda()
    tlp = logp.gather(-1, tok.unsqueeze(-1)).squeeze(-1)
    for i, row in enumerate(tok.tolist()):
        ln = row.index(cfg.eos_token_id) + 1 if cfg.eos_token_id in row else len(row)
        assert abs(float(tlp[i, :ln].sum()) / ln - float(sc[i])) < 1e-3 * (1 + abs(float(sc[i]))), (i, float(sc[i]))
    assert float(sc.view(B, k)[:, 0].min()) >= -1e30
    # sampling: every drawn token lies in HF's kept set of its teacher-forced logits (tests/sample_ref.py)
    t, tk, tp, n = 0.7, 5, 0.9, 3
    torch.manual_seed(5)
    ours = m.generate(pix, src, max_length=ml, do_sample=True, temperature=t, top_k=tk, top_p=tp, num_return_sequences=n).cpu()
    assert ours.shape[0] == B * n and (ours[:, 0] == cfg.decoder_start_token_id).all()
    lg = _teacher_forced_logits(m, pix, src, ours, n).cpu()
    rows, steps, V = lg.shape
    flat = lg.reshape(rows * steps, V)
    ok = ~torch.isinf(hf_warp(flat, t, tk, tp)) | boundary_tokens(flat, t, tk, tp)
    inside = ok.view(rows, steps, V).gather(-1, ours[:, 1:].unsqueeze(-1)).squeeze(-1)
    live = (ours[:, 1:] == cfg.eos_token_id).cumsum(1).cumsum(1) <= 1
    assert inside[live].all()
    # processors: each picked token is the arg-max of HF's processed teacher-forced logits (tests/logits_proc_ref.py)
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=4)
    out = m.generate(pix, src, max_length=ml, **kw).cpu()
    lg = _teacher_forced_logits(m, pix, src, out, 1).cpu()
    for s in range(out.shape[1] - 1):
        proc = hf_process(out[:, :s + 1], lg[:, s], eos_id=cfg.eos_token_id, **kw)
        top2 = proc.topk(2, -1).values
        for r in range(out.shape[0]):
            if (out[r, 1:s + 1] == cfg.eos_token_id).any() or float(top2[r, 0] - top2[r, 1]) < 1e-4:
                continue
            assert int(proc[r].argmax()) == int(out[r, s + 1]), (r, s)


# --------------------------------------------------------------------------------------------------- optimizer and checkpoints
def test_fused_adam_on_the_untied_model_matches_torch_adam():
    from klab_multimodalmodel_amd.optim import FusedAdam
    ms, opts = [], []
    for fused in (False, True):
        m, g = build_v11("tiny_v11_a", torch.float32, False)
        m = m.to("cuda")
        m._direct_grads = True
        m.transformer.eval()
        ps = list(m.transformer.parameters())
        opts.append(FusedAdam(ps, lr=3e-3) if fused else torch.optim.Adam(ps, lr=3e-3))
        ms.append(m)
    before = {n: p.detach().clone() for n, p in ms[1].transformer.named_parameters()}
    losses = [[], []]
    for _step in range(3):
        for k in (0, 1):
            loss = run(ms[k], g)
            loss.backward()
            opts[k].step()
            opts[k].zero_grad()
            losses[k].append(float(loss))
    assert opts[1]._fallback is None and opts[1]._fb_reason is None, opts[1]._fb_reason  # the one-kernel path really ran
    for a, b in zip(losses[0], losses[1]):
        assert abs(a - b) <= 2e-5 * abs(a) + 1e-6, losses
    worst = 0.0
    for (n0, p0), (n1, p1) in zip(ms[0].transformer.named_parameters(), ms[1].transformer.named_parameters()):
        assert n0 == n1
        worst = max(worst, rel_l2(p1.detach().cpu(), p0.detach().cpu()))
        assert not torch.equal(p1.detach(), before[n1]), n1  # every tensor moved, lm_head.weight and wi_0 / wi_1 included
    assert worst < 1e-5, worst
    t = ms[1].transformer
    up_head = t.get_parameter("lm_head.weight").detach() - before["lm_head.weight"]
    up_emb = t.get_parameter("shared.weight").detach() - before["shared.weight"]
    assert not torch.equal(up_head, up_emb) and float(up_head.abs().max()) > 0 and float(up_emb.abs().max()) > 0


def test_checkpoint_resume_on_the_untied_model_with_dropout(tmp_path):
    from klab_multimodalmodel_amd.checkpoint import AsyncCheckpointer, load_checkpoint
    from klab_multimodalmodel_amd.optim import FusedAdam

    def make(seed_base):
        m, g = build_v11("tiny_v11_a", torch.float32, False)
        m = m.to("cuda")
        m.args.result_dir = str(tmp_path)
        m._seed_base = seed_base
        m._direct_grads = True
        m.transformer.train()
        return m, g, FusedAdam(m.transformer.parameters(), lr=2e-3)

    def steps(m, g, opt, n):
        out = []
        for _ in range(n):
            loss = run(m, g)
            loss.backward()
            opt.step()
            opt.zero_grad()
            out.append(float(loss))
        return out

    m1, g, o1 = make(1234)
    first = steps(m1, g, o1, 2)
    assert len(set(first)) == 2
    ck = AsyncCheckpointer(str(tmp_path))
    ck.save(m1, o1, None, step=2, name="v11.pth")
    ck.wait()
    sd = torch.load(os.path.join(str(tmp_path), "v11.pth"), weights_only=False)["transformer"]
    assert "lm_head.weight" in sd and not torch.equal(sd["lm_head.weight"], sd["shared.weight"])
    cont = steps(m1, g, o1, 2)
    m2, g, o2 = make(999)  # another base: the checkpoint's must win
    run(m2, g)
    assert load_checkpoint(os.path.join(str(tmp_path), "v11.pth"), m2, o2) == 2
    rest = steps(m2, g, o2, 2)
    assert o2._fallback is None, o2._fb_reason
    # the step after the resume: same weights, same dropout masks (the gate's among them), a forward without atomics => the same bits
    assert rest[0] == cont[0], (rest, cont)
    assert abs(rest[1] - cont[1]) <= 2e-5 * abs(cont[1]) + 1e-6, (rest, cont)  # (behind one backward with f32 atomics)


# ----------------------------------------------------------------------------------------------------------- full-size properties
def _v11_small_model():
    """google/t5-v1_1-small (d_model 512, 6 heads x 64 = 384, d_ff 1024, 8 + 8 layers) with random weights behind a small Swin tower of
    the same width; the language encoder is t5-small"""
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.hf_io import KNOWN_T5
    from klab_multimodalmodel_amd.models.model import MyModel
    sw = SwinConfig(image_size=64, embed_dim=64, depths=(2, 2, 2, 2), num_heads=(2, 4, 8, 16), window_size=4)  # -> 512 wide, 4 image tokens
    lang = T5Config(**KNOWN_T5["t5-small"])
    main = T5Config(**KNOWN_T5["google/t5-v1_1-small"])
    return MyModel(args(), _configs=(sw, lang, main), _seed=3, dtype="bf16").to("cuda")


def test_v11_small_shape_properties():
    """B = 64, Ls 9, Lt 64, bf16: a finite eval loss that repeats bit for bit and is the mean of its half batches, and a finite
    train-mode step that leaves a finite, non-zero gradient in every tensor"""
    m = _v11_small_model()
    V = m.main_cfg.vocab_size
    B, Ls, Lt = 64, 9, 64
    g = torch.Generator().manual_seed(1)
    pix = torch.randn(B, 3, 64, 64, generator=g).cuda()
    src = torch.randint(2, V, (B, Ls), generator=g).cuda()
    tgt = torch.randint(2, V, (B, Lt), generator=g).cuda()

    def loss_of(sl, train=False):
        m.transformer.train(train)
        return m({"pixel_values": pix[sl]}, {"input_ids": src[sl]}, {"input_ids": tgt[sl]})

    with torch.no_grad():
        full = float(loss_of(slice(0, B)))
        again = float(loss_of(slice(0, B)))
        h0, h1 = float(loss_of(slice(0, B // 2))), float(loss_of(slice(B // 2, B)))
    print("v1.1-small eval loss", full, "ln(V)", math.log(V), "halves", h0, h1)
    assert math.isfinite(full) and full == again
    # HF's init gives the untied head N(0, 1) rows and v1.1 does not scale the decoder output, so a random model's logits have a
    # standard deviation of about sqrt(d_model) = 22.6 and its loss is ln(V) plus up to the expected maximum of V such logits,
    # sigma * sqrt(2 ln V) = 103 -- not the ln(V) of a v1.0 random init.  Below ln(V) - 1 it cannot be for random targets.
    sigma = math.sqrt(m.main_cfg.d_model)
    assert math.log(V) - 1.0 < full < math.log(V) + 1.2 * sigma * math.sqrt(2 * math.log(V)), full
    assert abs(0.5 * (h0 + h1) - full) <= 2e-3 * full
    loss = loss_of(slice(0, B), train=True)
    loss.backward()
    assert math.isfinite(float(loss))
    for n, p in m.transformer.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
