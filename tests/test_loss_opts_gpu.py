"""The cross-entropy with options on the GPU: klab_ce_wsum / klab_ce_fwd_opts (csrc/ce.hip) through `ops` against the plain
kernel (neutral options: bit for bit) and against the fp64 reference of tests/loss_opts_ref.py (per-element bounds), and
MyModel.set_loss_options / target_encoding["loss_weights"] / token_losses on golden tiny_a against the oracle's logits put through
the formula in torch.

rule                                                              -> shape
  the plain kernel's dispatch (one-pass NIT 8 | 16, two-pass; f32)  -> bf16 V = 8, 2056, 16384 | 16392, 32768 | 32776, 40000; f32 V = 4, 1028, 4104
  the sum and reduce kernels stride 256 threads over the rows       -> rows = 6 and 261
  row stride ld > V                                                 -> ld = V + 16 with sentinels behind every row"""
import types

import pytest
import torch

from tests import loss_opts_ref as LR
from tests import rowops_ref as R
from tests.helpers import cosine, load_golden, rel_l2
from tests.rowops_ref import CE_PAD, CE_SENT, CE_V, Guarded, assert_equal, assert_within

pytestmark = pytest.mark.gpu

F32 = torch.float32
CE_CASES = [(6, V, dt) for dt in ("bf16", "f32") for V in CE_V[dt]] + [(261, 2056, "bf16"), (261, 1028, "f32")]
OPTIONS = [(0.1, 0.0), (0.0, 0.05), (0.3, 0.05)]
KEYS = ("logits", "inv", "loss_row", "loss")


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


def run_kernel(ops, c, V, write_grad, eps=None, z=0.0, weights=None, sum_first=False):
    """eps None: the plain klab_ce_fwd (the yardstick); otherwise klab_ce_fwd_opts.  Everything between guard bands."""
    rows = c["stored"].shape[0]
    ld = V + CE_PAD
    image = torch.full((rows, ld), CE_SENT, dtype=c["dtype"])
    image[:, :V] = c["stored"]
    buf = Guarded((rows, ld), c["dtype"], init=image)
    inv, loss_row, loss = Guarded((1,), F32), Guarded((rows,), F32), Guarded((1,), F32)
    labels = c["labels"].cuda()
    w = None if weights is None else weights.cuda()
    if eps is None:
        ops.ce_fwd(buf.t[:, :V], labels, inv.t, loss_row.t, loss.t, write_grad=write_grad)
    else:
        if sum_first:
            ops.ce_wsum(labels, w, inv.t)
        ops.ce_fwd_opts(buf.t[:, :V], labels, w, inv.t, loss_row.t, loss.t, eps=eps, z=z, write_grad=write_grad)
    torch.cuda.synchronize()
    return dict(image=image, logits=buf.check("logits"), inv=inv.check("inv"), loss_row=loss_row.check("loss_row"), loss=loss.check("loss"))


@pytest.mark.parametrize("rows,V,dt", CE_CASES)
def test_neutral_options_are_the_plain_kernel_bit_for_bit(ops, rows, V, dt):
    c = R.ce_case(rows, V, dt)
    tag = f" rows={rows} V={V} {dt}"
    plain = {wg: run_kernel(ops, c, V, wg) for wg in (False, True)}
    for name, w in (("no weights", None), ("weights all ones", torch.ones(rows))):
        for wg in (False, True):
            got = run_kernel(ops, c, V, wg, eps=0.0, z=0.0, weights=w)
            for k in KEYS:
                assert_equal(f"ce_fwd_opts {k} ({name}, write_grad={wg})", got[k], plain[wg][k], tag)
            if not wg:
                assert_equal(f"ce_fwd_opts logits left intact ({name})", got["logits"], got["image"], tag)


@pytest.mark.parametrize("rows,V,dt", CE_CASES)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps,z", OPTIONS)
def test_options_match_fp64_within_the_derived_bounds(ops, rows, V, dt, eps, z, weighted):
    c = LR.opts_case(rows, V, dt, eps, z, weighted)
    tag = f" rows={rows} V={V} {dt} eps={eps} z={z} weights={weighted}"
    w, valid = c["weights"], c["valid"]
    a = run_kernel(ops, c, V, False, eps=eps, z=z, weights=w)
    assert_equal("ce_fwd_opts logits (write_grad = False)", a["logits"], a["image"], tag)
    assert_within("ce_wsum inv_w", a["inv"], c["inv_w"].reshape(1), c["inv_w_bound"].reshape(1), tag)
    assert_within("ce_fwd_opts loss_row", a["loss_row"], c["loss_row"], c["row_bound"], tag)
    assert bool((a["loss_row"][~valid] == 0).all()), f"loss_row{tag}: a row without a label has a loss"
    assert_within("ce_fwd_opts loss", a["loss"], c["loss"].reshape(1), c["loss_bound"].reshape(1), tag)
    b = run_kernel(ops, c, V, True, eps=eps, z=z, weights=w)
    assert_equal("ce_fwd_opts sentinel columns behind V", b["logits"][:, V:], a["image"][:, V:], tag)
    grad = b["logits"][:, :V]
    assert bool((grad[~valid] == 0).all()), f"gradient{tag}: a row without a label has a gradient"
    if weighted:
        dead = valid & (w == 0)
        assert bool(dead.any()) and bool((grad[dead] == 0).all()), f"gradient{tag}: a row of weight 0 has a gradient"
        assert bool((b["loss_row"][dead] != 0).all()), f"loss_row{tag}: a row of weight 0 must still get its loss"
    assert_within("ce_fwd_opts gradient", grad, c["grad"], c["gbound"], tag)
    assert_equal("ce_fwd_opts loss_row (with gradient)", b["loss_row"], a["loss_row"], tag)
    assert_equal("ce_fwd_opts loss (with gradient)", b["loss"], a["loss"], tag)
    d = run_kernel(ops, c, V, 3, eps=eps, z=z, weights=w, sum_first=True)  # inv_w summed ahead of the logits
    e = run_kernel(ops, c, V, True, eps=eps, z=z, weights=w)               # a second run
    for k in KEYS:
        assert_equal(f"ce_fwd_opts {k} (write_grad | 2 after ce_wsum)", d[k], b[k], tag)
        assert_equal(f"ce_fwd_opts {k} (second run)", e[k], b[k], tag)


@pytest.mark.parametrize("rows,V,dt", [(6, 2056, "bf16"), (6, 32768, "bf16"), (6, 40000, "bf16"), (261, 1028, "f32")])
def test_all_weights_zero(ops, rows, V, dt):
    c = R.ce_case(rows, V, dt)
    got = run_kernel(ops, c, V, True, eps=0.3, z=0.05, weights=torch.zeros(rows))
    assert float(got["inv"]) == 0.0 and float(got["loss"]) == 0.0
    assert bool((got["logits"][:, :V] == 0).all()) and not bool(torch.isnan(got["loss_row"]).any())
    assert_equal("sentinel columns", got["logits"][:, V:], got["image"][:, V:])
    assert bool((got["loss_row"][c["valid"]] != 0).all())


@pytest.mark.parametrize("V,dt", [(2052, "bf16"), (1030, "f32")])
def test_a_width_off_the_vector_is_refused_and_nothing_is_written(ops, V, dt):
    dtype = torch.bfloat16 if dt == "bf16" else F32
    rows, ld = 6, V + CE_PAD
    image = torch.full((rows, ld), CE_SENT, dtype=dtype)
    buf = Guarded((rows, ld), dtype, init=image)
    inv, loss_row, loss = Guarded((1,), F32), Guarded((rows,), F32), Guarded((1,), F32)
    labels = torch.zeros(rows, dtype=torch.int64).cuda()
    with pytest.raises(NotImplementedError):
        ops.ce_fwd_opts(buf.t[:, :V], labels, torch.ones(rows).cuda(), inv.t, loss_row.t, loss.t, eps=0.1, z=0.05, write_grad=True)
    torch.cuda.synchronize()
    assert_equal("logits", buf.check("logits"), image)
    for g, name in ((inv, "inv_w"), (loss_row, "loss_row"), (loss, "loss")):
        assert bool(torch.isnan(g.check(name)).all()), f"{name} was written by a refused call"


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
# The tolerances are the project's.  Every case first proves, in the reference alone, that its options move the
# loss by 100 loss tolerances and the gradient by 1e-2 (rel-L2): a forward that ignored them could not pass.  For fp32 (tolerance
# 2e-5) eps = 0.1, z = 0.05 and weights that zero the pads and double the first sample do that on the golden batch.  bf16 tolerates
# 2e-3, so the loss has to move by 20 %:
#   z        0.05 moves it by 36 % (lse is about 7: z lse^2 = 2.4 on a loss of 6.6)
#   weights  zeroed pads and a doubled sample move the mean of the 21 token losses (0.7 ... 9.2) by 5 %, whatever the factor; "hard"
#            weights -- 3 on the tokens whose reference loss is >= 8, 0.25 on the others, 0 on the pads -- move it by 21 %
#   eps      moves a token's loss by eps (mean_j x_j - x_y), 3.6 % of the golden batch's loss even at eps = 0.99 (the random model's
#            labels are as likely as any token).  On the batch's LEAST likely labels (position by position the arg-min of the
#            oracle's logits, x_y about 3 below the mean) eps = 0.7 moves it by 22 %: the bf16 smoothing case uses those labels
EPS, Z = 0.1, 0.05
LOSS_TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-3}
HARD_LOSS = 8.0
MODEL_CASES = {  # name -> dtype -> (eps, z, weights kind, labels kind)
    "smoothing": {torch.float32: (EPS, 0.0, None, "golden"), torch.bfloat16: (0.7, 0.0, None, "unlikely")},
    "z": {torch.float32: (0.0, Z, None, "golden"), torch.bfloat16: (0.0, Z, None, "golden")},
    "weights": {torch.float32: (0.0, 0.0, "hard", "golden"), torch.bfloat16: (0.0, 0.0, "hard", "golden")},
    "all": {torch.float32: (EPS, Z, "sample", "golden"), torch.bfloat16: (EPS, Z, "sample", "golden")},
}


def build(name="tiny_a", dtype=torch.float32, train_swin=False, train=False):
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_golden(name)
    sw, t5 = SwinConfig.from_dict(g["meta"]["swin_config"]), T5Config.from_dict(g["meta"]["t5_config"])
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=train_swin,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], g["sds"]["main"]), dtype=dtype).to("cuda")
    m._direct_grads = True
    m.transformer.train(train)
    return m, g


def run(m, g, weights=None, tgt_ids=None):
    inp = g["inputs"]
    tgt = {"input_ids": (inp["tgt_ids"] if tgt_ids is None else tgt_ids).cuda()}
    if weights is not None:
        tgt["loss_weights"] = weights
    return m({"pixel_values": inp["pixel_values"].cuda()}, {"input_ids": inp["src_ids"].cuda()}, tgt)


def model_weights(g):
    """zero on the pad tokens, the first sample doubled (fp32 [B, Lt] on the host)"""
    tgt = g["inputs"]["tgt_ids"]
    w = (tgt != g["t5_cfg"].pad_token_id).float()
    w[0] *= 2.0
    return w


class Oracle:
    """the oracle's logits of tiny_a (one forward per set of labels, its graph kept and never written) and, through the fp32 torch
    statement of the formula, reference(eps, z, weights kind, labels kind) -> (loss, {name: gradient})"""

    def __init__(self):
        from oracle import swin_t5_oracle as O
        self.O = O
        self.g = g = load_golden("tiny_a")
        self.main = {k: v.clone().requires_grad_(True) for k, v in g["sds"]["main"].items()}
        self.tgt, self.logits, self.cache = {"golden": g["inputs"]["tgt_ids"]}, {}, {}

    def forward(self, tgt_ids, main):
        g = self.g
        sds, inp = g["sds"], g["inputs"]
        return self.O.mymodel_forward(sds["swin"], sds["lang"], main, g["swin_cfg"], g["t5_cfg"], g["t5_cfg"], inp["pixel_values"], inp["src_ids"],
                                      tgt_ids, training=False, return_parts=True)[1]["logits"]

    def labels(self, kind):
        if kind not in self.tgt:  # "unlikely": the decoder is causal, so position i's arg-min depends on the labels before it only
            t = self.g["inputs"]["tgt_ids"].clone()
            with torch.no_grad():
                for i in range(t.shape[1]):
                    t[:, i] = self.forward(t, self.g["sds"]["main"])[:, i].argmin(-1)
            self.tgt[kind] = t
        return self.tgt[kind]

    def weights(self, kind):
        if kind is None or kind == "sample":
            return None if kind is None else model_weights(self.g)
        lg = self._logits("golden").detach()
        tgt = self.labels("golden")
        l = LR.reference(lg.reshape(-1, lg.shape[-1]), tgt.reshape(-1))["loss_row"].view(tgt.shape)
        w = torch.where(l >= HARD_LOSS, 3.0, 0.25).float()
        return w * (tgt != self.g["t5_cfg"].pad_token_id)

    def _logits(self, kind):
        if kind not in self.logits:
            self.logits[kind] = self.forward(self.labels(kind), self.main)
        return self.logits[kind]

    def reference(self, eps=0.0, z=0.0, weights=None, labels="golden"):
        key = (eps, z, weights, labels)
        if key not in self.cache:
            lg, w = self._logits(labels), self.weights(weights)
            loss = LR.torch_loss(lg.reshape(-1, lg.shape[-1]), self.labels(labels).reshape(-1), eps, z, None if w is None else w.reshape(-1))
            names = list(self.main)
            grads = torch.autograd.grad(loss, [self.main[k] for k in names], retain_graph=True, allow_unused=True)
            self.cache[key] = (float(loss.detach()), {k: gr for k, gr in zip(names, grads) if gr is not None})
        return self.cache[key]


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def flat(grads, keys):
    return torch.cat([grads[k].flatten().double() for k in keys])


def native_grads(m):
    return {k: p.grad.detach().cpu() for k, p in m.transformer.named_parameters() if p.grad is not None}


def assert_token_losses(m, loss, tgt, w):
    """token_losses() is [B, Lt] and sum w l / W of it is the loss the forward returned"""
    tl = m.token_losses()
    assert tuple(tl.shape) == tuple(tgt.shape) and tl.dtype == torch.float32 and tl.is_cuda
    ww = (w.cpu() if w is not None else torch.ones(tgt.shape)).double() * (tgt != -100)
    assert abs(float((ww * tl.cpu().double()).sum() / ww.sum()) - float(loss)) <= 1e-6 * abs(float(loss))
    assert bool((tl.cpu()[tgt == -100] == 0).all())


def bite(oracle, tol, eps, z, wkind, lkind):
    """the condition, in the reference alone; returns the optioned reference"""
    plain_loss, plain_grads = oracle.reference(labels=lkind)
    want_loss, want_grads = oracle.reference(eps, z, wkind, lkind)
    keys = sorted(want_grads)
    shift = abs(want_loss - plain_loss) / abs(plain_loss)
    gshift = rel_l2(flat(want_grads, keys), flat(plain_grads, keys))
    print(f"reference: plain {plain_loss:.6f}, with options {want_loss:.6f}: loss moves by {shift:.4f} (needs {100 * tol}), gradient by {gshift:.4f}")
    assert shift >= 100 * tol, (want_loss, plain_loss)
    assert gshift >= 1e-2, gshift
    return want_loss, want_grads, keys


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_model_matches_the_oracle_through_the_formula(oracle, dtype, case):
    eps, z, wkind, lkind = MODEL_CASES[case][dtype]
    g, tol = oracle.g, LOSS_TOL[dtype]
    want_loss, want_grads, keys = bite(oracle, tol, eps, z, wkind, lkind)
    m, _ = build("tiny_a", dtype)
    m.set_loss_options(label_smoothing=eps, z_loss=z)
    assert m.loss_options == {"label_smoothing": eps, "z_loss": z}
    w = oracle.weights(wkind)
    w = None if w is None else w.cuda()
    tgt = oracle.labels(lkind)
    loss = run(m, g, w, tgt)
    print("loss", float(loss), "reference", want_loss)
    assert abs(float(loss) - want_loss) <= tol * abs(want_loss), (float(loss), want_loss)
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
    assert_token_losses(m, loss, tgt, w)


def test_options_in_training_mode_repeat_with_the_seed(oracle):
    g = oracle.g
    out = []
    for _ in range(2):
        torch.manual_seed(1234)
        m, _g = build("tiny_a", train=True)
        m.set_loss_options(label_smoothing=EPS, z_loss=Z)
        w = model_weights(g).cuda()
        loss = run(m, g, w)
        tl = m.token_losses().cpu().double()
        ww = w.cpu().double() * (g["inputs"]["tgt_ids"] != -100)
        assert abs(float((ww * tl).sum() / ww.sum()) - float(loss)) <= 1e-6 * abs(float(loss))
        out.append(float(loss))
    torch.manual_seed(1234)
    p, _g = build("tiny_a", train=True)
    plain = float(run(p, g))
    assert out[0] == out[1] and torch.isfinite(torch.tensor(out[0])) and out[0] != plain, (out, plain)


ATOMIC = ("shared.weight", "relative_attention_bias.weight")


def test_back_to_neutral_is_the_plain_model_bit_for_bit(oracle):
    """After set_loss_options() back to neutral the model issues the plain launches again: the loss, the per-token losses, d logits
    (the whole output of the cross-entropy, which the unchanged backward consumes) and every gradient equal those of a model that
    never set an option, bit for bit -- but for the three tensors that float atomics write, whose bits the plain model does not
    repeat against ITSELF (five fresh plain models on an MI355X: shared.weight -- the tied table's scatter-add, the start token's
    row collects one add per sample -- and the two relative_attention_bias tables differed in every pair of runs, nothing else in
    any).  For those the project's rule for atomics applies (tests/test_wgrad_store_engine_gpu.py): the distance to a plain run
    stays within twice the largest distance between plain runs, with a floor of 2^-22 of the tensor's norm (four units in the
    last place) for the day the plain runs happen to agree."""
    g = oracle.g
    plains = []
    for _ in range(3):
        p, _g = build("tiny_a")
        loss = run(p, g)
        loss.backward()
        plains.append(dict(loss=loss.detach().cpu(), tl=p.token_losses().cpu(), dlogits=p._engine.buffer("logits").clone().cpu(), grads=native_grads(p)))
    p0 = plains[0]
    # token_losses works on a model that never set an option (tiny_a scores every token: the plain loss is their mean)
    assert tuple(p0["tl"].shape) == tuple(g["inputs"]["tgt_ids"].shape)
    assert abs(float(p0["tl"].double().mean()) - float(p0["loss"])) <= 1e-6 * abs(float(p0["loss"]))
    m, _g = build("tiny_a")
    m.set_loss_options(label_smoothing=EPS, z_loss=Z)
    run(m, g, model_weights(g).cuda()).backward()
    m.zero_grad(set_to_none=True)
    m.set_loss_options()
    assert m.loss_options == {"label_smoothing": 0.0, "z_loss": 0.0}
    # weights of all ones: the plain loss, bit for bit
    ones = run(m, g, torch.ones(g["inputs"]["tgt_ids"].shape, device="cuda"))
    assert_equal("loss (weights all ones)", ones.detach().cpu(), p0["loss"])
    ones.backward()
    assert_equal("d logits (weights all ones)", m._engine.buffer("logits").clone().cpu(), p0["dlogits"])
    m.zero_grad(set_to_none=True)
    again = run(m, g)
    again.backward()
    assert_equal("loss (back to neutral)", again.detach().cpu(), p0["loss"])
    assert_equal("token_losses (back to neutral)", m.token_losses().cpu(), p0["tl"])
    assert_equal("d logits (back to neutral)", m._engine.buffer("logits").clone().cpu(), p0["dlogits"])
    mg = native_grads(m)
    assert set(mg) == set(p0["grads"])
    dist = lambda a, b: float((a.double() - b.double()).norm())
    for k, ref in p0["grads"].items():
        if k.endswith(ATOMIC):
            spread = max(dist(plains[i]["grads"][k], plains[j]["grads"][k]) for i, j in ((0, 1), (0, 2), (1, 2)))
            allowed = max(2.0 * spread, 2.0 ** -22 * float(ref.double().norm()))
            print(f"{k}: distance to a plain run {dist(mg[k], ref):.3e}, between plain runs {spread:.3e}")
            assert dist(mg[k], ref) <= allowed, (k, dist(mg[k], ref), spread)
        else:
            for q in plains[1:]:  # the yardstick repeats itself here
                assert_equal(f"gradient {k} (plain against plain)", q["grads"][k], ref)
            assert_equal(f"gradient {k} (back to neutral)", mg[k], ref)


def test_bad_weights_are_refused_and_leave_nothing_armed(oracle):
    g = oracle.g
    m, _g = build("tiny_a")
    plain = float(run(m, g))
    shape = tuple(g["inputs"]["tgt_ids"].shape)
    for bad in (torch.ones(shape[0], shape[1] + 1, device="cuda"), torch.ones(shape[0] * shape[1], device="cuda"), torch.ones(shape),
                torch.ones(shape, dtype=torch.int64, device="cuda")):
        with pytest.raises(ValueError):
            run(m, g, bad)
        assert float(run(m, g)) == plain


def test_gradient_accumulation_keeps_the_fused_optimizer(oracle):
    from klab_multimodalmodel_amd.optim import FusedAdamW
    g = oracle.g
    m, _g = build("tiny_a")
    m.set_loss_options(label_smoothing=EPS, z_loss=Z)
    opt = FusedAdamW(m.transformer.parameters(), lr=1e-3)
    w = model_weights(g).cuda()
    before = [p.detach().clone() for p in m.transformer.parameters()]
    for _ in range(2):
        run(m, g, w).backward()
    opt.step()
    assert opt._fallback is None and opt._fb_reason is None, opt._fb_reason
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, m.transformer.parameters()))


def test_graph_replay_does_not_bake_the_options_in(oracle):
    g = oracle.g
    m, _g = build("tiny_a")
    m.use_graph = True
    order = (0.1, 0.3, 0.1, 0.3)  # (a graph slot runs eagerly once, is captured at its second use and replayed from the third)
    got = []
    for eps in order:
        m.set_loss_options(label_smoothing=eps)
        got.append(float(run(m, g)))
    want = {eps: oracle.reference(eps)[0] for eps in set(order)}
    assert abs(want[0.1] - want[0.3]) >= 100 * 2e-5 * abs(want[0.1])  # a replayed eps could not pass
    for eps, v in zip(order, got):
        assert abs(v - want[eps]) <= 2e-5 * abs(want[eps]), (eps, got, want)
