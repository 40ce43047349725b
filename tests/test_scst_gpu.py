"""Self-critical training on the GPU: klab_ciderd_rewards against the fp64 reference of tests/scst_ref.py within the tolerance fixed
there, klab_scst_targets bit for bit, the count-normalised signed loss on golden tiny_a against the oracle's logits put through the
formula (the project's parity thresholds: fp32 loss 2e-5 and gradients 1e-4 rel-L2, bf16 loss 2e-3 and cosine 0.99), and
scst.SelfCritical end to end.

rule                                                          -> shape
  lane i owns the n-gram that starts at unit i, one wave64      -> 1, 3, 4, 63 and 64 units
  eight waves stride over the references and the hypotheses     -> R = 1, 5, 16; n_h = 1, 5
  one workgroup per image                                       -> B = 1, 2, 3
  the targets kernel strides 64 lanes over Lt, one wave per row -> L = 2, 5, 65 with Lt = L - 1 and L + 70; 1, 2, 5, 10 rows"""
import numpy as np
import pytest
import torch

from tests import scst_ref as S
from tests.helpers import cosine, rel_l2
from tests.rowops_ref import Guarded, assert_equal, assert_within
from tests.test_loss_opts_gpu import LOSS_TOL, Oracle, build, flat, native_grads, run
from tests.test_scst_cpu import build_table

pytestmark = pytest.mark.gpu

F32 = torch.float32
EOS = S.EOS


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


# ---- rewards ---------------------------------------------------------------------------------------------------------------------------
def kernel_rewards(ops, c, table):
    hyp, refs = c["hyp"].cuda(), c["refs"].cuda()
    out = Guarded((hyp.shape[0],), F32)
    ops.ciderd_rewards(hyp, refs, table.keys, table.idf, table.log_n, out.t, n_h=c["n_h"], sigma=table.sigma, eos=EOS,
                       count_eos=table.count_eos)
    torch.cuda.synchronize()
    return out.check("rewards")


@pytest.mark.parametrize("name", list(S.reward_cases()))
def test_rewards_match_fp64_within_the_fixed_tolerance(ops, name):
    c = S.reward_cases()[name]
    table = build_table(c).to("cuda")
    want = torch.from_numpy(S.case_reference(c))
    got = kernel_rewards(ops, c, table)
    print(name, "reference", want.tolist())
    assert_within("ciderd_rewards", got, want, S.REWARD_TOL, f" {name}")
    # exact zeros: no present reference, no units
    refs, hyp = c["refs"], c["hyp"]
    for r in range(hyp.shape[0]):
        if bool((refs[r // c["n_h"], :, 0] < 0).all()) or not S.units(hyp[r, 1:].tolist(), EOS, c["count_eos"]):
            assert float(got[r]) == 0.0 and float(want[r]) == 0.0, (name, r, float(got[r]))
    assert_equal("ciderd_rewards (second run)", kernel_rewards(ops, c, table), got)


def test_rewards_through_the_public_function(ops):
    from klab_multimodalmodel_amd import scst
    c = S.reward_cases()["batch count_eos=True"]
    table = build_table(c).to("cuda")
    got = scst.ciderd(table, c["hyp"].cuda(), c["refs"].cuda())
    assert tuple(got.shape) == (3, 5) and got.dtype == F32
    assert_equal("scst.ciderd", got.cpu().reshape(-1), kernel_rewards(ops, c, table))


def test_unsupported_shapes_are_refused_and_nothing_is_written(ops):
    c = S.reward_cases()["one reference"]
    table = build_table(c).to("cuda")
    out = Guarded((2,), F32)
    for hyp, refs in ((torch.zeros(2, 66, dtype=torch.int64), c["refs"]), (c["hyp"], torch.zeros(2, 1, 65, dtype=torch.int64)),
                      (c["hyp"], torch.zeros(2, 17, 8, dtype=torch.int64))):
        with pytest.raises(NotImplementedError):
            ops.ciderd_rewards(hyp.cuda(), refs.cuda(), table.keys, table.idf, table.log_n, out.t, n_h=1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.check("rewards")).all())


# ---- targets ---------------------------------------------------------------------------------------------------------------------------
def target_case(B, n, L, seed):
    """sequences with and without EOS (one row closes at its first generated token, one never), rewards k / 8"""
    g = torch.Generator().manual_seed(seed)
    rows = B * n
    seq = torch.randint(2, 50, (rows, L), generator=g)
    seq[:, 0] = S.START
    for r in range(rows):
        if r % 3 != 1:  # every third row has no EOS
            e = 1 + (r * 5) % (L - 1)
            seq[r, e] = EOS
            seq[r, e + 1:] = S.PAD
            if r % 2 and e + 2 < L:
                seq[r, e + 2] = EOS  # a second EOS behind the first changes nothing
    rew = torch.randint(0, 81, (rows,), generator=g).float() / 8.0
    base = torch.randint(0, 81, (B,), generator=g).float() / 8.0
    return seq, rew, base


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,n", [(1, 1), (1, 2), (2, 5)])
@pytest.mark.parametrize("L,extra", [(2, 0), (5, 0), (5, 3), (65, 0), (65, 70)])
def test_targets_bit_for_bit(ops, mode, B, n, L, extra):
    if mode == 1 and n < 2:
        seq, rew, base = target_case(B, n, L, 3)
        with pytest.raises(ValueError):
            ops.scst_targets(seq.cuda(), rew.cuda(), None, torch.empty(B * n, L - 1, dtype=torch.int64, device="cuda"),
                             torch.empty(B * n, L - 1, device="cuda"), torch.empty(B * n, device="cuda"), n=n, mode=1)
        return
    seq, rew, base = target_case(B, n, L, 11 * L + n)
    Lt = L - 1 + extra
    want = S.targets(seq, rew, base, mode, n, Lt)
    lab, w, adv = Guarded((B * n, Lt), torch.int64), Guarded((B * n, Lt), F32), Guarded((B * n,), F32)
    ops.scst_targets(seq.cuda(), rew.cuda(), base.cuda() if mode == 0 else None, lab.t, w.t, adv.t, n=n, mode=mode)
    torch.cuda.synchronize()
    tag = f" mode={mode} B={B} n={n} L={L} Lt={Lt}"
    assert_equal("labels", lab.check("labels"), want[0], tag)
    assert_equal("weights", w.check("weights"), want[1], tag)
    assert_equal("advantages", adv.check("advantages"), want[2], tag)


def test_targets_refuse_a_short_lt(ops):
    seq, rew, base = target_case(1, 2, 5, 1)
    with pytest.raises(ValueError):
        ops.scst_targets(seq.cuda(), rew.cuda(), None, torch.empty(2, 3, dtype=torch.int64, device="cuda"), torch.empty(2, 3, device="cuda"),
                         torch.empty(2, device="cuda"), n=2, mode=2)


# ---- the count-normalised, signed loss -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def signed_weights(g):
    """advantage-like: one value per caption, of both signs, summing to little ([B, Lt] fp32 on the host)"""
    tgt = g["inputs"]["tgt_ids"]
    return torch.tensor([1.5, -2.0, 0.75])[:tgt.shape[0]].view(-1, 1).expand(tgt.shape).contiguous()


def count_reference(oracle, w, eps=0.0):
    """(loss, grads, scale) of sum w l / N through the oracle's logits; scale = sum |w| l / N, the size of the terms that cancel in the
    signed sum: the project's relative loss tolerances are applied to it (relative to the sum itself they would tighten with every
    advantage that happens to cancel another)"""
    lg = oracle._logits("golden")
    tgt = oracle.labels("golden").reshape(-1)
    x = lg.reshape(-1, lg.shape[-1])
    lse = torch.logsumexp(x, -1)
    l = lse - (1.0 - eps) * x[torch.arange(x.shape[0]), tgt.clamp_min(0)] - (eps / x.shape[1]) * x.sum(-1)
    valid = tgt != -100
    loss = (torch.where(valid, w.reshape(-1) * l, torch.zeros_like(l))).sum() / valid.sum()
    names = list(oracle.main)
    grads = torch.autograd.grad(loss, [oracle.main[k] for k in names], retain_graph=True, allow_unused=True)
    scale = float((torch.where(valid, w.reshape(-1).abs() * l, torch.zeros_like(l))).sum().detach() / valid.sum())
    return float(loss.detach()), {k: gr for k, gr in zip(names, grads) if gr is not None}, scale


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_count_norm_with_signed_weights_matches_the_oracle(oracle, dtype, eps):
    g, tol = oracle.g, LOSS_TOL[dtype]
    w = signed_weights(g)
    want_loss, want_grads, scale = count_reference(oracle, w, eps)
    keys = sorted(want_grads)
    sum_loss = oracle.reference(eps, 0.0, None)[0]
    # the reference alone: the signed count-normalised loss is far from the plain one, and sum w is no usable normaliser
    assert abs(want_loss - sum_loss) >= 100 * tol * abs(sum_loss) and abs(float(w.sum())) < 0.1 * float(w.abs().sum())
    m, _ = build("tiny_a", dtype)
    m.set_loss_options(label_smoothing=eps, weight_norm="count")
    assert m.loss_options == {"label_smoothing": eps, "z_loss": 0.0, "weight_norm": "count"}
    loss = run(m, g, w.cuda())
    print("loss", float(loss), "reference", want_loss)
    assert abs(float(loss) - want_loss) <= tol * scale, (float(loss), want_loss, scale)
    tl = m.token_losses().cpu().double()
    assert abs(float((w.double() * tl).sum() / w.numel()) - float(loss)) <= 1e-6 * scale
    loss.backward()
    assert int(m._engine.err_view.item()) == 0
    got = native_grads(m)
    if dtype == torch.float32:
        for k in keys:
            if float(want_grads[k].abs().max()) == 0.0:
                continue
            assert rel_l2(got[k], want_grads[k]) <= 1e-4, (k, rel_l2(got[k], want_grads[k]))
    else:
        c = cosine(flat(got, keys), flat(want_grads, keys))
        print("gradient cosine", c)
        assert c >= 0.99, c


def test_all_ones_under_count_and_back_at_sum_are_the_plain_bits(oracle):
    g = oracle.g
    p, _ = build("tiny_a")
    plain = run(p, g)
    plain.backward()
    want = dict(loss=plain.detach().cpu(), tl=p.token_losses().cpu(), dlogits=p._engine.buffer("logits").clone().cpu())
    pw, _ = build("tiny_a")  # the weighted "sum" path of a model that never heard of weight_norm
    w = signed_weights(g).abs()
    sum_loss = run(pw, g, w.cuda())
    sum_loss.backward()
    want_sum = dict(loss=sum_loss.detach().cpu(), dlogits=pw._engine.buffer("logits").clone().cpu())

    m, _ = build("tiny_a")
    m.set_loss_options(weight_norm="count")
    for name, weights in (("weights all ones", torch.ones(g["inputs"]["tgt_ids"].shape, device="cuda")), ("no weights", None)):
        loss = run(m, g, weights)
        assert_equal(f"loss under count ({name})", loss.detach().cpu(), want["loss"])
        loss.backward()
        assert_equal(f"d logits under count ({name})", m._engine.buffer("logits").clone().cpu(), want["dlogits"])
        m.zero_grad(set_to_none=True)
    run(m, g, signed_weights(g).cuda()).backward()  # a signed step in between
    m.zero_grad(set_to_none=True)
    m.set_loss_options()
    assert m.loss_options == {"label_smoothing": 0.0, "z_loss": 0.0}
    again = run(m, g)
    again.backward()
    assert_equal("loss (back at sum)", again.detach().cpu(), want["loss"])
    assert_equal("token_losses (back at sum)", m.token_losses().cpu(), want["tl"])
    assert_equal("d logits (back at sum)", m._engine.buffer("logits").clone().cpu(), want["dlogits"])
    m.zero_grad(set_to_none=True)
    ws = run(m, g, w.cuda())
    ws.backward()
    assert_equal("weighted loss (back at sum)", ws.detach().cpu(), want_sum["loss"])
    assert_equal("weighted d logits (back at sum)", m._engine.buffer("logits").clone().cpu(), want_sum["dlogits"])


def test_count_norm_grouped_with_label_smoothing_and_with_lora(oracle):
    """[B, n, Lt] labels: the loss is the 2-D call's on the images repeated; with LoRA the adapters get the gradient, and negated
    weights negate loss and gradients (g = w / N is signed arithmetic all the way)"""
    from klab_multimodalmodel_amd import lora
    g = oracle.g
    inp = g["inputs"]
    n = 2
    tgt = torch.stack([inp["tgt_ids"], inp["tgt_ids"].flip(0)], 1).contiguous()  # [B, 2, Lt]
    w = torch.tensor([[1.5, -0.5], [-2.0, 0.25], [0.75, -1.0]]).view(3, 2, 1).expand(tgt.shape).contiguous()
    images, source = {"pixel_values": inp["pixel_values"].cuda()}, {"input_ids": inp["src_ids"].cuda()}
    m, _ = build("tiny_a")
    m.set_loss_options(label_smoothing=0.1, weight_norm="count")
    grouped = m(images, source, {"input_ids": tgt.cuda(), "loss_weights": w.cuda()})
    tl = m.token_losses().cpu().double()
    assert tuple(tl.shape) == tuple(tgt.shape)
    scale = float((w.abs().double() * tl).sum() / w.numel())
    assert abs(float((w.double() * tl).sum() / w.numel()) - float(grouped)) <= 1e-6 * scale
    flat2 = m({"pixel_values": images["pixel_values"].repeat_interleave(n, 0)}, {"input_ids": source["input_ids"].repeat_interleave(n, 0)},
              {"input_ids": tgt.view(-1, tgt.shape[-1]).cuda(), "loss_weights": w.view(-1, w.shape[-1]).cuda()})
    assert abs(float(flat2) - float(grouped)) <= 2e-5 * scale, (float(flat2), float(grouped))

    ad = lora.attach(m, r=4, alpha=16, targets=("q", "v"), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        for k, p in ad.named_parameters():
            if ".lora_B." in k:
                p.copy_((0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(6))).to(p.device))
    out = {}
    for sign in (1.0, -1.0):
        for p in ad.parameters():
            p.grad = None
        loss = m(images, source, {"input_ids": tgt.cuda(), "loss_weights": (sign * w).cuda()})
        loss.backward()
        assert int(m._engine.err_view.item()) == 0
        out[sign] = (float(loss), torch.cat([p.grad.flatten().double().cpu() for p in ad.parameters()]))
    assert float(out[1.0][1].norm()) > 0 and bool(torch.isfinite(out[1.0][1]).all())
    assert abs(out[1.0][0] + out[-1.0][0]) <= 1e-6 * scale
    assert rel_l2(-out[-1.0][1], out[1.0][1]) <= 1e-6


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def scst_setup(dtype=torch.float32):
    """tiny_a, references drawn from the model itself under another seed (three per image, the last absent for image 1), the corpus
    and its table"""
    from klab_multimodalmodel_amd import scst
    m, g = build("tiny_a", dtype)
    inp = g["inputs"]
    pixels, src = inp["pixel_values"].cuda(), inp["src_ids"].cuda()
    torch.manual_seed(101)
    drawn = m.generate(pixels, src, max_length=9, do_sample=True, num_return_sequences=3, top_k=3).cpu()
    B = src.shape[0]
    refs = torch.full((B, 3, 8), -100, dtype=torch.int64)
    lists = []
    for b in range(B):
        lists.append([])
        for j in range(3):
            u = S.units(drawn[b * 3 + j, 1:].tolist())
            if b == 1 and j == 2:
                continue
            refs[b, j, :len(u)] = torch.tensor(u)
            lists[-1].append(u)
    # five more images of a corpus, so that an n-gram all three images share still weighs log(8 / 3)
    corpus = lists + [[[300 + i, 301 + i, EOS]] for i in range(5)]
    table = scst.CiderD.from_references(corpus, vocab_size=m.main_cfg.vocab_size, eos_token_id=EOS).to("cuda")
    return m, {"pixel_values": pixels}, {"input_ids": src}, refs, corpus, table


@pytest.mark.parametrize("baseline", ["greedy", "mean", "none"])
def test_self_critical_is_its_hand_composition(baseline):
    """The loss equals, bit for bit, generate + the targets reference + the model's own weighted forward under weight_norm="count",
    fed the rewards as tensors; the rewards themselves are held to the fp64 reference within the reward tolerance (an fp32 kernel
    cannot promise an fp64 reference's bits, so the composition takes the tensors the step computed)."""
    from klab_multimodalmodel_amd import scst
    m, images, source, refs, corpus, table = scst_setup()
    n, max_length = 4, 9
    sc = scst.SelfCritical(m, table, samples=n, baseline=baseline, max_length=max_length, top_k=3)
    m.set_loss_options(label_smoothing=0.1)
    torch.manual_seed(7)
    loss, info = sc.loss(images, source, refs.cuda())
    assert m.loss_options == {"label_smoothing": 0.1, "z_loss": 0.0}  # weight_norm was "count" for that call only
    loss.backward()
    dlogits = m._engine.buffer("logits").clone().cpu()
    B = refs.shape[0]
    # the same sessions by hand
    torch.manual_seed(7)
    seq = m.generate(images["pixel_values"], source["input_ids"], max_length=max_length, do_sample=True, num_return_sequences=n, top_k=3)
    assert_equal("sequences", info["sequences"].cpu(), seq.cpu())
    df, N = S.doc_freq(corpus), len(corpus)
    want_r = S.rewards(seq.cpu(), refs, n, df, N)
    assert_within("rewards", info["rewards"].reshape(-1), torch.from_numpy(want_r), S.REWARD_TOL)
    assert float(np.abs(want_r).max()) > 0.1, "the samples share nothing with the references: the step trains on nothing"
    base = None
    if baseline == "greedy":
        greedy = m.generate(images["pixel_values"], source["input_ids"], max_length=max_length)
        assert_within("baseline", info["baseline"], torch.from_numpy(S.rewards(greedy.cpu(), refs, 1, df, N)), S.REWARD_TOL)
        base = info["baseline"].cpu()
    else:
        assert info["baseline"] is None
    labels, weights, adv = S.targets(seq.cpu(), info["rewards"].reshape(-1).cpu(), base, scst.BASELINES[baseline], n, max_length - 1)
    assert_equal("advantages", info["advantages"].cpu().reshape(-1), adv)
    assert bool((adv > 0).any()) and bool((adv < 0).any()) or baseline == "none"
    m.zero_grad(set_to_none=True)
    m.set_loss_options(label_smoothing=0.1, weight_norm="count")
    hand = m(images, source, {"input_ids": labels.view(B, n, -1).cuda(), "loss_weights": weights.view(B, n, -1).cuda()})
    hand.backward()
    assert_equal("loss", loss.detach().cpu(), hand.detach().cpu())
    assert_equal("d logits", dlogits, m._engine.buffer("logits").clone().cpu())


def test_two_calls_with_one_seed_agree_and_the_mode_is_restored():
    from klab_multimodalmodel_amd import scst
    m, images, source, refs, _lists, table = scst_setup(torch.bfloat16)
    sc = scst.SelfCritical(m, table, samples=3, baseline="greedy", max_length=9, top_k=3)
    out = []
    for _ in range(2):
        torch.manual_seed(21)
        with torch.no_grad():
            loss, info = sc.loss(images, source, refs.cuda())
        out.append((loss.cpu(), info["rewards"].cpu(), info["advantages"].cpu(), info["sequences"].cpu()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert not m.transformer.training
    m.transformer.train()
    sc.loss(images, source, refs.cuda())
    assert m.transformer.training  # the sampling ran in eval mode and the mode came back


def test_the_users_weight_norm_survives_an_exception():
    from klab_multimodalmodel_amd import scst
    m, images, source, refs, _lists, table = scst_setup()
    sc = scst.SelfCritical(m, table, samples=2, baseline="none", max_length=9, top_k=3)
    m.set_loss_options(z_loss=1e-4)
    real = m.forward

    def failing(*a, **k):
        assert m.loss_options.get("weight_norm") == "count"
        raise RuntimeError("inside the call")

    m.forward = failing
    with pytest.raises(RuntimeError, match="inside the call"):
        sc.loss(images, source, refs.cuda())
    m.forward = real
    assert m.loss_options == {"label_smoothing": 0.0, "z_loss": 1e-4}
    m.set_loss_options(weight_norm="count")
    sc.loss(images, source, refs.cuda())
    assert m.loss_options == {"label_smoothing": 0.0, "z_loss": 0.0, "weight_norm": "count"}
