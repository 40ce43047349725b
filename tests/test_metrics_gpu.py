"""Caption metrics on the GPU: klab_caption_stats bit for bit against the Counter / LCS-table reference of tests/metrics_ref.py (integer
outputs: no tolerance), metrics.sentence_scores on the device against the `math` formulas at rel 1e-12 (both sides are about a dozen
IEEE-double operations with pow / exp within a few ulp), and scst.SelfCritical's reward mixing on the tiny model of
tests/test_scst_gpu.py against the public functions, bit for bit.

rule                                                              -> shape
  lane i owns the n-gram that starts at unit i, one wave64          -> 0, 1, 3, 4 (the first guess_4 = 1), 63 and 64 units; 65 columns
  one LDS word per reference unit serves the four orders            -> a 4-id vocabulary, ids 2 and 65534, junk behind the EOS
  eight waves stride over the references and the hypotheses         -> R = 1, 5, 16 with absent ones; n_h = 1, 5, 9
  one workgroup per image                                           -> B = 1, 2, 3, 7
  the LCS word is masked to the reference's length                  -> references of 0, 3, 5 and 64 units
  ties are decided by index and by integer cross-multiplication    -> the case "ties" """
import pytest
import torch

from tests import metrics_ref as M
from tests.rowops_ref import Guarded, assert_equal

pytestmark = pytest.mark.gpu

EOS = M.EOS
I32 = torch.int32


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


def kernel_stats(ops, c):
    hyp, refs = c["hyp"].cuda(), c["refs"].cuda()
    out = Guarded((hyp.shape[0], 16), I32)
    ops.caption_stats(hyp, refs, out.t, n_h=c["n_h"], eos=EOS, count_eos=c["count_eos"])
    torch.cuda.synchronize()
    return out.check("stats")


@pytest.mark.parametrize("name", list(M.cases()))
def test_kernel_integers_equal_the_reference(ops, name):
    c = M.cases()[name]
    want = M.case_reference(name)
    got = kernel_stats(ops, c)
    assert_equal("caption_stats", got, want, f" {name}")
    assert_equal("caption_stats (second run)", kernel_stats(ops, c), got, f" {name}")


def test_anchor_rows_on_the_device(ops):
    hyps = list(M.ANCHORS)
    hyp = torch.tensor([M.hyp_row(M.ids(h), 9) for h in hyps])
    refs = torch.tensor([[M.ref_row(M.ids(r), 8) for r in M.ANCHOR_REFS]] * len(hyps))
    got = kernel_stats(ops, dict(hyp=hyp, refs=refs, n_h=1, count_eos=False))
    assert got.tolist() == [M.ANCHORS[h][0] + [0, 0] for h in hyps]


def test_the_public_function_is_the_kernel(ops):
    from klab_multimodalmodel_amd import metrics
    c = M.cases()["batch count_eos=True"]
    got = metrics.caption_stats(c["hyp"].cuda(), c["refs"].cuda(), EOS, True)
    assert tuple(got.shape) == (7, 5, 16) and got.dtype == I32 and got.is_cuda
    assert_equal("metrics.caption_stats", got.cpu().view(-1, 16), M.case_reference("batch count_eos=True"))
    one = M.cases()["one reference"]
    got = metrics.caption_stats(one["hyp"].cuda(), one["refs"].cuda())  # [B, L]: n = 1
    assert tuple(got.shape) == (3, 1, 16)
    assert_equal("metrics.caption_stats [B, L]", got.cpu().view(-1, 16), M.case_reference("one reference"))
    with pytest.raises(ValueError):
        metrics.caption_stats(one["hyp"].cuda(), one["refs"])  # the references on another device


def test_unsupported_shapes_are_refused_and_nothing_is_written(ops):
    c = M.cases()["one reference"]
    out = Guarded((3, 16), I32)
    i64 = torch.int64
    for hyp, refs in ((torch.zeros(3, 66, dtype=i64), c["refs"]), (c["hyp"], torch.zeros(3, 1, 65, dtype=i64)),
                      (c["hyp"], torch.zeros(3, 17, 8, dtype=i64))):
        with pytest.raises(NotImplementedError):
            ops.caption_stats(hyp.cuda(), refs.cuda(), out.t, n_h=1)
    torch.cuda.synchronize()
    assert bool((out.check("stats") == -1).all())


def test_sentence_scores_on_the_device():
    from klab_multimodalmodel_amd import metrics
    rows = torch.cat([M.case_reference(name) for name in M.cases()])
    got = metrics.sentence_scores(rows.cuda())
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (rows.shape[0], 5)
    got = got.cpu()
    want = torch.tensor([M.sentence(r) for r in rows.tolist()], dtype=torch.float64)
    err = (got - want).abs()
    print("largest relative error", float((err / want.abs().clamp_min(1e-300)).max()), "over", rows.shape[0], "rows")
    assert bool((err <= 1e-12 * want.abs()).all()), (err / want.abs().clamp_min(1e-300)).max()
    assert bool((got[rows[:, 13] == 0] == 0).all()) and bool((want > 0).any(0).all())
    beta = metrics.sentence_scores(rows.cuda(), beta=2.0).cpu()[:, 4]
    want_b = torch.tensor([M.rouge_l(r, 2.0) if r[13] else 0.0 for r in rows.tolist()], dtype=torch.float64)
    assert bool(((beta - want_b).abs() <= 1e-12 * want_b.abs()).all())


def test_caption_metrics_on_the_device():
    from klab_multimodalmodel_amd import metrics
    from tests.test_metrics_cpu import corpus_batches
    batches = corpus_batches(False)
    want = M.corpus([r for hyp, refs in batches for r in M.stats(hyp, refs, 1).tolist()])
    cm = metrics.CaptionMetrics()
    for hyp, refs in batches:
        cm.update(hyp.cuda(), refs.cuda())
    assert cm.sums.is_cuda and tuple(cm.sums.shape) == (12,)
    got = cm.compute()
    assert got["images"] == want["images"] == 8
    for k in M.NAMES:
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])


# ---- reward mixing in SelfCritical -------------------------------------------------------------------------------------------------------
def test_a_cider_only_mixture_is_scst_ciderd():
    from klab_multimodalmodel_amd import scst
    from tests.test_scst_gpu import scst_setup
    m, images, source, refs, _corpus, table = scst_setup()
    sc = scst.SelfCritical(m, table, samples=3, baseline="greedy", max_length=9, top_k=3, reward_weights={"ciderd": 1.0})
    torch.manual_seed(7)
    loss, info = sc.loss(images, source, refs.cuda())
    want = scst.ciderd(table, info["sequences"], refs.cuda())
    assert_equal("rewards", info["rewards"], want)
    assert list(info["reward_terms"]) == ["ciderd"]
    assert_equal("reward_terms['ciderd']", info["reward_terms"]["ciderd"], want)
    plain = scst.SelfCritical(m, table, samples=3, baseline="greedy", max_length=9, top_k=3)
    torch.manual_seed(7)
    loss0, info0 = plain.loss(images, source, refs.cuda())
    assert "reward_terms" not in info0
    for k in ("sequences", "rewards", "baseline", "advantages"):
        assert_equal(k, info[k], info0[k])
    assert_equal("loss", loss.detach(), loss0.detach())


def test_a_mixture_is_the_public_functions_and_trains():
    from klab_multimodalmodel_amd import metrics, scst
    from tests.test_scst_gpu import scst_setup
    m, images, source, refs, _corpus, table = scst_setup()
    n, w = 4, {"ciderd": 1.0, "bleu4": 0.5, "rouge_l": 0.25}
    sc = scst.SelfCritical(m, table, samples=n, baseline="greedy", max_length=9, top_k=3, reward_weights=w)
    torch.manual_seed(7)
    loss, info = sc.loss(images, source, refs.cuda())
    refs_d = refs.cuda()

    def mixture(seq):
        scores = metrics.sentence_scores(metrics.caption_stats(seq, refs_d, table.eos_token_id, table.count_eos))
        return (1.0 * scst.ciderd(table, seq, refs_d).double() + 0.5 * scores[..., 3] + 0.25 * scores[..., 4]).float(), scores

    want, scores = mixture(info["sequences"])
    assert info["rewards"].dtype == torch.float32 and tuple(info["rewards"].shape) == (refs.shape[0], n)
    assert_equal("rewards", info["rewards"], want)
    assert sorted(info["reward_terms"]) == ["bleu4", "ciderd", "rouge_l"]
    assert_equal("reward_terms['bleu4']", info["reward_terms"]["bleu4"], scores[..., 3])
    assert_equal("reward_terms['rouge_l']", info["reward_terms"]["rouge_l"], scores[..., 4])
    assert float(scores[..., 4].max()) > 0.1, "the samples share nothing with the references"
    greedy = m.generate(images["pixel_values"], source["input_ids"], max_length=9)
    base = mixture(greedy)[0].view(-1)
    assert_equal("baseline", info["baseline"], base)
    assert_equal("advantages", info["advantages"], info["rewards"] - base.view(-1, 1))
    assert bool(torch.isfinite(loss)) and float(info["advantages"].abs().max()) > 0
    loss.backward()
    assert int(m._engine.err_view.item()) == 0
    grads = [p.grad for p in m.transformer.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
    # a term with weight 0 is not computed
    only = scst.SelfCritical(m, table, samples=2, baseline="none", max_length=9, top_k=3, reward_weights={"ciderd": 0.0, "rouge_l": 2.0})
    torch.manual_seed(7)
    _loss, info = only.loss(images, source, refs_d)
    assert list(info["reward_terms"]) == ["rouge_l"]
    sc2 = metrics.sentence_scores(metrics.caption_stats(info["sequences"], refs_d, table.eos_token_id, table.count_eos))
    assert_equal("rewards (rouge_l alone)", info["rewards"], (2.0 * sc2[..., 4]).float())
