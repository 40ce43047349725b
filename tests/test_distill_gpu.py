"""Knowledge distillation in the loss on the GPU: klab_ce_fwd_distill (csrc/ce.hip) through `ops` against klab_ce_fwd_opts
(alpha = 0: bit for bit) and against the fp64 reference of tests/distill_ref.py (per-element bounds), and
MyModel.set_loss_options(distill_alpha, distill_temperature) / target_encoding["teacher_logits"] / token_kl / logits /
distill.teacher_logits on golden tiny_a against the oracle's logits put through the formula in torch.

rule                                                              -> shape
  the dispatch (one-pass NIT 8 | 16, two-pass; f32 student)         -> bf16 V = 8, 2056, 16384 | 16392, 32768 | 32776, 40000; f32 V = 4, 1028, 4104
  the sum and reduce kernels stride 256 threads over the rows       -> rows = 6 and 261
  row strides ld, ldt > V                                           -> ld = V + 16, ldt = V + 24, sentinels behind every row of both
  the teacher's own dtype and 16-byte vector                        -> bf16 and f32 teachers for either student; an f32 student's width
                                                                       off the bf16 teacher's vector (V = 4, 1028) must be refused"""
import types

import pytest
import torch

from tests import distill_ref as DR
from tests import loss_opts_ref as LR
from tests.helpers import cosine, load_golden, rel_l2
from tests.rowops_ref import CE_PAD, CE_SENT, CE_V, Guarded, assert_equal, assert_within

pytestmark = pytest.mark.gpu

F32 = torch.float32
T_PAD, T_SENT = 24, 555.0
SHAPES = [(6, V, dt) for dt in ("bf16", "f32") for V in CE_V[dt]] + [(261, 2056, "bf16"), (261, 1028, "f32")]
CASES = [(rows, V, dt, tdt) for rows, V, dt in SHAPES for tdt in ("bf16", "f32")]
KEYS = ("logits", "inv", "loss_row", "loss")


def fits(V, tdt):
    return V % DR.teacher_vector(tdt) == 0


RUN = [c for c in CASES if fits(c[1], c[3])]
OFF = [c for c in CASES if not fits(c[1], c[3])]
SAME = [c for c in RUN if not (c[2] == "f32" and c[3] == "bf16")]  # (an f32 row does not survive a bf16 teacher)


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


class Buffers:
    """student logits, teacher and every output between guard bands; rows of both matrices end in sentinel columns"""

    def __init__(self, stored, teacher, V):
        rows = stored.shape[0]
        self.V, self.rows = V, rows
        self.image = torch.full((rows, V + CE_PAD), CE_SENT, dtype=stored.dtype)
        self.image[:, :V] = stored
        self.timage = torch.full((rows, V + T_PAD), T_SENT, dtype=teacher.dtype)
        self.timage[:, :V] = teacher
        self.buf = Guarded((rows, V + CE_PAD), stored.dtype, init=self.image)
        self.tbuf = Guarded((rows, V + T_PAD), teacher.dtype, init=self.timage)
        self.inv, self.loss_row, self.kl_row, self.loss = Guarded((1,), F32), Guarded((rows,), F32), Guarded((rows,), F32), Guarded((1,), F32)

    def read(self):
        torch.cuda.synchronize()
        assert_equal("the teacher and its sentinels", self.tbuf.check("teacher"), self.timage)
        return dict(image=self.image, logits=self.buf.check("logits"), inv=self.inv.check("inv"), loss_row=self.loss_row.check("loss_row"),
                    kl_row=self.kl_row.check("kl_row"), loss=self.loss.check("loss"))

    def untouched(self):
        torch.cuda.synchronize()
        assert_equal("logits", self.buf.check("logits"), self.image)
        assert_equal("teacher", self.tbuf.check("teacher"), self.timage)
        for g, name in ((self.inv, "inv_w"), (self.loss_row, "loss_row"), (self.kl_row, "kl_row"), (self.loss, "loss")):
            assert bool(torch.isnan(g.check(name)).all()), f"{name} was written by a refused call"


def run_distill(ops, c, V, write_grad, eps, z, weights, alpha, T, sum_first=False):
    b = Buffers(c["stored"], c["teacher"], V)
    labels = c["labels"].cuda()
    w = None if weights is None else weights.cuda()
    if sum_first:
        ops.ce_wsum(labels, w, b.inv.t)
    ops.ce_fwd_distill(b.buf.t[:, :V], b.tbuf.t[:, :V], labels, w, b.inv.t, b.loss_row.t, b.kl_row.t, b.loss.t, eps=eps, z=z, alpha=alpha,
                       temperature=T, write_grad=write_grad)
    return b.read()


def run_opts(ops, c, V, write_grad, eps, z, weights):
    rows = c["stored"].shape[0]
    image = torch.full((rows, V + CE_PAD), CE_SENT, dtype=c["dtype"])
    image[:, :V] = c["stored"]
    buf = Guarded((rows, V + CE_PAD), c["dtype"], init=image)
    inv, loss_row, loss = Guarded((1,), F32), Guarded((rows,), F32), Guarded((1,), F32)
    w = None if weights is None else weights.cuda()
    ops.ce_fwd_opts(buf.t[:, :V], c["labels"].cuda(), w, inv.t, loss_row.t, loss.t, eps=eps, z=z, write_grad=write_grad)
    torch.cuda.synchronize()
    return dict(logits=buf.check("logits"), inv=inv.check("inv"), loss_row=loss_row.check("loss_row"), loss=loss.check("loss"))


@pytest.mark.parametrize("rows,V,dt,tdt", RUN)
def test_alpha_zero_is_the_options_kernel_bit_for_bit(ops, rows, V, dt, tdt):
    tag = f" rows={rows} V={V} {dt} teacher={tdt}"
    for eps, z in DR.OPTIONS:
        for weighted in (False, True):
            c = DR.distill_case(rows, V, dt, tdt, eps, z, weighted, 0.5, 1.0)
            for wg in (False, True):
                want = run_opts(ops, c, V, wg, eps, z, c["weights"])
                for T in (1.0, 2.0):
                    got = run_distill(ops, c, V, wg, eps, z, c["weights"], 0.0, T)
                    for k in KEYS:
                        assert_equal(f"ce_fwd_distill {k} (alpha=0 T={T} eps={eps} z={z} weights={weighted} write_grad={wg})", got[k], want[k], tag)


def check_case(ops, c, V, eps, z, alpha, T, tag):
    w, valid = c["weights"], c["valid"]
    a = run_distill(ops, c, V, False, eps, z, w, alpha, T)
    assert_equal("ce_fwd_distill logits (write_grad = False)", a["logits"], a["image"], tag)
    assert_within("ce_wsum inv_w", a["inv"], c["inv_w"].reshape(1), c["inv_w_bound"].reshape(1), tag)
    assert_within("ce_fwd_distill kl_row", a["kl_row"], c["kl_row"], c["kl_bound"], tag)
    assert_within("ce_fwd_distill loss_row", a["loss_row"], c["loss_row"], c["row_bound"], tag)
    assert bool((a["loss_row"][~valid] == 0).all()) and bool((a["kl_row"][~valid] == 0).all()), f"{tag}: a row without a label has a loss"
    assert_within("ce_fwd_distill loss", a["loss"], c["loss"].reshape(1), c["loss_bound"].reshape(1), tag)
    b = run_distill(ops, c, V, True, eps, z, w, alpha, T)
    assert_equal("ce_fwd_distill sentinel columns behind V", b["logits"][:, V:], a["image"][:, V:], tag)
    grad = b["logits"][:, :V]
    assert bool((grad[~valid] == 0).all()), f"gradient{tag}: a row without a label has a gradient"
    if w is not None:
        dead = valid & (w == 0)
        assert bool(dead.any()) and bool((grad[dead] == 0).all()), f"gradient{tag}: a row of weight 0 has a gradient"
        scored = dead & (c["loss_row"] != 0)  # (alpha = 1 with the teacher equal to the student: the loss itself is 0)
        assert bool((b["loss_row"][scored] != 0).all()), f"loss_row{tag}: a row of weight 0 must still get its loss"
    assert_within("ce_fwd_distill gradient", grad, c["grad"], c["gbound"], tag)
    for k in ("loss_row", "kl_row", "loss"):
        assert_equal(f"ce_fwd_distill {k} (with gradient)", b[k], a[k], tag)
    return a, b


@pytest.mark.parametrize("rows,V,dt,tdt", RUN)
@pytest.mark.parametrize("alpha,T", DR.SETTINGS)
def test_distillation_matches_fp64_within_the_derived_bounds(ops, rows, V, dt, tdt, alpha, T):
    for eps, z in DR.OPTIONS:
        for weighted in (False, True):
            c = DR.distill_case(rows, V, dt, tdt, eps, z, weighted, alpha, T)
            tag = f" rows={rows} V={V} {dt} teacher={tdt} alpha={alpha} T={T} eps={eps} z={z} weights={weighted}"
            _a, b = check_case(ops, c, V, eps, z, alpha, T, tag)
            if (eps, weighted) == (0.3, True):  # inv_w summed ahead of the logits; a second run
                d = run_distill(ops, c, V, 3, eps, z, c["weights"], alpha, T, sum_first=True)
                e = run_distill(ops, c, V, True, eps, z, c["weights"], alpha, T)
                for k in KEYS + ("kl_row",):
                    assert_equal(f"ce_fwd_distill {k} (write_grad | 2 after ce_wsum)", d[k], b[k], tag)
                    assert_equal(f"ce_fwd_distill {k} (second run)", e[k], b[k], tag)


@pytest.mark.parametrize("rows,V,dt,tdt", SAME)
@pytest.mark.parametrize("alpha,T", DR.SETTINGS)
def test_a_teacher_equal_to_the_student_adds_nothing(ops, rows, V, dt, tdt, alpha, T):
    """kl_row within its bound of 0 and the gradient within its bound of (1 - alpha) x the cross-entropy's: at alpha = 1 its
    magnitude is bounded by the derived error term alone (the reference is exactly zero there)"""
    for eps, z, weighted in ((0.0, 0.0, False), (0.3, 0.05, True)):
        c = DR.distill_case(rows, V, dt, tdt, eps, z, weighted, alpha, T, True)
        assert bool((c["kl_row"] == 0).all()) and torch.equal(c["grad"], (1.0 - alpha) * c["ce_grad"])
        if alpha == 1.0:
            assert bool((c["grad"] == 0).all())
        check_case(ops, c, V, eps, z, alpha, T, f" rows={rows} V={V} {dt} teacher={tdt} (= student) alpha={alpha} T={T} eps={eps} weights={weighted}")


def refusal_buffers(V, dt, tdt, rows=6):
    dtype, tdtype = DR.TDTYPE[dt], DR.TDTYPE[tdt]
    b = Buffers(torch.zeros(rows, V, dtype=dtype), torch.ones(rows, V, dtype=tdtype), V)
    return b, torch.zeros(rows, dtype=torch.int64).cuda(), torch.ones(rows).cuda()


def call(ops, b, labels, w, V, alpha=0.5, T=2.0, logits=None, teacher=None):
    ops.ce_fwd_distill(b.buf.t[:, :V] if logits is None else logits, b.tbuf.t[:, :V] if teacher is None else teacher, labels, w, b.inv.t,
                       b.loss_row.t, b.kl_row.t, b.loss.t, eps=0.1, z=0.05, alpha=alpha, temperature=T, write_grad=True)


@pytest.mark.parametrize("V,dt,tdt", [(2052, "bf16", "bf16"), (2052, "bf16", "f32"), (1030, "f32", "f32"), (1030, "f32", "bf16")]
                         + [(V, dt, tdt) for _r, V, dt, tdt in OFF if _r == 6])
def test_a_width_off_either_vector_is_refused_and_nothing_is_written(ops, V, dt, tdt):
    b, labels, w = refusal_buffers(V, dt, tdt)
    with pytest.raises(NotImplementedError):
        call(ops, b, labels, w, V)
    b.untouched()


@pytest.mark.parametrize("dt,tdt", [("bf16", "bf16"), ("bf16", "f32"), ("f32", "f32"), ("f32", "bf16")])
def test_bad_options_and_overlapping_ranges_are_refused_and_nothing_is_written(ops, dt, tdt):
    V = 2056
    b, labels, w = refusal_buffers(V, dt, tdt)
    for kw in (dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=float("nan")), dict(T=0.0), dict(T=-1.0), dict(T=float("inf")), dict(T=float("nan"))):
        with pytest.raises(ValueError):
            call(ops, b, labels, w, V, **kw)
    b.untouched()
    # both matrices carved out of one arena (byte offsets): the same start, the teacher beginning inside the student's range, the
    # student beginning inside the teacher's
    es, tes, rows = (2 if dt == "bf16" else 4), (2 if tdt == "bf16" else 4), 6
    ld, ldt = V + CE_PAD, V + T_PAD
    arena = torch.zeros(4 * rows * ldt * 4, dtype=torch.uint8, device="cuda")
    before = arena.clone()

    def carve(off, nbytes, dtype, stride):
        return arena[off:off + nbytes].view(dtype).view(rows, stride)[:, :V]

    for xo, to in ((0, 0), (0, 4096), (4096, 0), (0, ((rows - 1) * ld + V) * es - 16), (((rows - 1) * ldt + V) * tes - 16, 0)):
        with pytest.raises(ValueError):
            call(ops, b, labels, w, V, logits=carve(xo, rows * ld * es, DR.TDTYPE[dt], ld), teacher=carve(to, rows * ldt * tes, DR.TDTYPE[tdt], ldt))
        torch.cuda.synchronize()
        assert torch.equal(arena, before), "a refused call wrote into the arena"
    b.untouched()
    # ranges that only touch are accepted: the student begins where the teacher's last row ends
    call(ops, b, labels, w, V, logits=carve(((rows - 1) * ldt + V) * tes, rows * ld * es, DR.TDTYPE[dt], ld),
         teacher=carve(0, rows * ldt * tes, DR.TDTYPE[tdt], ldt))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(b.loss.check("loss")).all()) and bool(torch.isfinite(b.kl_row.check("kl_row")).all())


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
# The tolerances are the project's (tests/test_loss_opts_gpu.py uses the same for the options): loss 2e-5 / 2e-3,
# fp32 gradients rel-L2 1e-4 per tensor, bf16 gradients cosine 0.99 overall.  Every case first proves, in the reference alone, that
# distillation moves the loss by 100 loss tolerances and the gradient by 1e-2 (rel-L2): a forward that ignored the teacher could
# not pass.
LOSS_TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-3}
ALPHA, TEMP = 0.5, 2.0
EPS, Z = 0.1, 0.05
ATOMIC = ("shared.weight", "relative_attention_bias.weight")


def build(name="tiny_a", dtype=torch.float32, train=False, main=None):
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_golden(name)
    sw, t5 = SwinConfig.from_dict(g["meta"]["swin_config"]), T5Config.from_dict(g["meta"]["t5_config"])
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], g["sds"]["main"] if main is None else main),
                dtype=dtype).to("cuda")
    m._direct_grads = True
    m.transformer.train(train)
    return m, g


def encodings(g, teacher=None, weights=None, tgt_ids=None):
    inp = g["inputs"]
    tgt = {"input_ids": (inp["tgt_ids"] if tgt_ids is None else tgt_ids).cuda()}
    if weights is not None:
        tgt["loss_weights"] = weights
    if teacher is not None:
        tgt["teacher_logits"] = teacher
    return {"pixel_values": inp["pixel_values"].cuda()}, {"input_ids": inp["src_ids"].cuda()}, tgt


def run(m, g, teacher=None, weights=None, tgt_ids=None):
    return m(*encodings(g, teacher, weights, tgt_ids))


def model_weights(g):
    """zero on the pad tokens, the first sample doubled (fp32 [B, Lt] on the host)"""
    tgt = g["inputs"]["tgt_ids"]
    w = (tgt != g["t5_cfg"].pad_token_id).float()
    w[0] *= 2.0
    return w


def second_main(g):
    """the weights of a second tiny model: tiny_a's trainable T5 with every floating-point tensor moved by 20 % noise"""
    gen = torch.Generator().manual_seed(77)
    return {k: (v + 0.2 * v.std() * torch.randn(v.shape, generator=gen) if v.is_floating_point() and v.numel() > 1 else v.clone())
            for k, v in g["sds"]["main"].items()}


class Oracle:
    """the oracle's logits of tiny_a (graph kept and never written), the logits of the second tiny model, a fixed random teacher, and
    reference(...) -> (loss, token losses, token kl, {name: gradient}) through the fp32 torch statement of the formula"""

    def __init__(self):
        from oracle import swin_t5_oracle as O
        self.O = O
        self.g = g = load_golden("tiny_a")
        self.main = {k: v.clone().requires_grad_(True) for k, v in g["sds"]["main"].items()}
        self.tgt = g["inputs"]["tgt_ids"]
        self.logits = self.forward(self.main)
        B, Lt, V = self.logits.shape
        self.teachers = {"random": 2.0 * torch.randn(B, Lt, V, generator=torch.Generator().manual_seed(5))}
        with torch.no_grad():
            self.teachers["second"] = self.forward(second_main(g)).detach()
        self.cache = {}

    def forward(self, main):
        g = self.g
        sds, inp = g["sds"], g["inputs"]
        return self.O.mymodel_forward(sds["swin"], sds["lang"], main, g["swin_cfg"], g["t5_cfg"], g["t5_cfg"], inp["pixel_values"], inp["src_ids"],
                                      self.tgt, training=False, return_parts=True)[1]["logits"]

    def reference(self, teacher=None, alpha=0.0, T=1.0, eps=0.0, z=0.0, weighted=False):
        key = (teacher, alpha, T, eps, z, weighted)
        if key not in self.cache:
            lg = self.logits
            V = lg.shape[-1]
            w = model_weights(self.g).reshape(-1) if weighted else None
            x, lab = lg.reshape(-1, V), self.tgt.reshape(-1)
            if teacher is None:
                loss = LR.torch_loss(x, lab, eps, z, w)
                tl = kl = None
            else:
                t = self.teachers[teacher].reshape(-1, V)
                loss = DR.torch_loss(x, t, lab, eps, z, w, alpha, T)
                r = DR.reference(x.detach(), t, lab, eps, z, w, alpha, T)
                tl, kl = r["loss_row"].view(self.tgt.shape), r["kl_row"].view(self.tgt.shape)
            names = list(self.main)
            grads = torch.autograd.grad(loss, [self.main[k] for k in names], retain_graph=True, allow_unused=True)
            self.cache[key] = (float(loss.detach()), tl, kl, {k: gr for k, gr in zip(names, grads) if gr is not None})
        return self.cache[key]


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def flat(grads, keys):
    return torch.cat([grads[k].flatten().double() for k in keys])


def native_grads(m):
    return {k: p.grad.detach().cpu() for k, p in m.transformer.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", ["random", "second", "random with options"])
def test_model_matches_the_oracle_through_the_formula(oracle, dtype, case):
    from klab_multimodalmodel_amd import distill
    g, tol = oracle.g, LOSS_TOL[dtype]
    kind = "second" if case == "second" else "random"
    eps, z, weighted = (EPS, Z, True) if case == "random with options" else (0.0, 0.0, False)
    plain_loss, _tl, _kl, plain_grads = oracle.reference(None, eps=eps, z=z, weighted=weighted)
    want_loss, want_tl, want_kl, want_grads = oracle.reference(kind, ALPHA, TEMP, eps, z, weighted)
    keys = sorted(want_grads)
    shift, gshift = abs(want_loss - plain_loss) / abs(plain_loss), rel_l2(flat(want_grads, keys), flat(plain_grads, keys))
    print(f"reference: plain {plain_loss:.6f}, distilled {want_loss:.6f}: loss moves by {shift:.4f} (needs {100 * tol}), gradient by {gshift:.4f}")
    assert shift >= 100 * tol and gshift >= 1e-2, (want_loss, plain_loss, gshift)
    m, _ = build("tiny_a", dtype)
    m.set_loss_options(label_smoothing=eps, z_loss=z, distill_alpha=ALPHA, distill_temperature=TEMP)
    assert m.loss_options == {"label_smoothing": eps, "z_loss": z, "distill_alpha": ALPHA, "distill_temperature": TEMP}
    if kind == "second":  # the teacher's logits come from a second native model, in its compute dtype, read in place
        tm, _ = build("tiny_a", dtype, train=True, main=second_main(g))
        teacher = distill.teacher_logits(tm, *encodings(g), student=m)
        assert tm.transformer.training and teacher.dtype == dtype and teacher.data_ptr() == tm._engine.buffer("logits").data_ptr()
        err, cs = rel_l2(teacher.float().cpu(), oracle.teachers["second"]), cosine(teacher.float().cpu(), oracle.teachers["second"])
        print("teacher logits against the oracle's: rel-L2", err, "cosine", cs)
        assert err <= 1e-4 if dtype == torch.float32 else cs >= 0.99
    else:
        teacher = oracle.teachers["random"].to(dtype).cuda()
    before = teacher.clone()
    w = model_weights(g).cuda() if weighted else None
    loss = run(m, g, teacher, w)
    print("loss", float(loss), "reference", want_loss)
    assert abs(float(loss) - want_loss) <= tol * abs(want_loss), (float(loss), want_loss)
    tl, kl = m.token_losses(), m.token_kl()
    assert tuple(kl.shape) == tuple(oracle.tgt.shape) and kl.dtype == torch.float32 and kl.is_cuda
    print("token losses rel-L2", rel_l2(tl.cpu(), want_tl), "token kl rel-L2", rel_l2(kl.cpu(), want_kl))
    if dtype == torch.float32:  # per-token vectors by the project's rule for vectors: fp32 rel-L2, bf16 cosine (the mean is the loss above)
        assert rel_l2(tl.cpu(), want_tl) <= tol and rel_l2(kl.cpu(), want_kl) <= tol, (rel_l2(tl.cpu(), want_tl), rel_l2(kl.cpu(), want_kl))
    else:
        assert cosine(tl.cpu(), want_tl) >= 0.99 and cosine(kl.cpu(), want_kl) >= 0.99, (cosine(tl.cpu(), want_tl), cosine(kl.cpu(), want_kl))
    assert bool((kl.cpu()[oracle.tgt == -100] == 0).all()) and bool((tl.cpu()[oracle.tgt == -100] == 0).all())
    ww = (w.cpu() if w is not None else torch.ones(oracle.tgt.shape)).double() * (oracle.tgt != -100)
    assert abs(float((ww * tl.cpu().double()).sum() / ww.sum()) - float(loss)) <= 1e-6 * abs(float(loss))
    with pytest.raises(RuntimeError, match="no_grad"):
        m.logits()  # this forward wrote d logits in place
    loss.backward()
    assert int(m._engine.err_view.item()) == 0
    assert torch.equal(teacher, before), "the teacher's logits were written"
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


def total_norm(m):
    return float(torch.cat([p.grad.detach().flatten().double() for p in m.transformer.parameters() if p.grad is not None]).norm())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_self_distillation_has_no_gradient(oracle, dtype):
    """alpha = 1, the teacher the model's own no-grad logits: the reference gradient is exactly zero, so d logits is bounded element by
    element by distill_ref's gbound and the cross-entropy's d logits of the same batch is the yardstick.  The backward is linear in
    d logits, so the factor the kernel-level bound implies is ||gbound||_2 / ||d logits of the plain loss||_2, computed from
    distill_ref on the model's own logits; the total gradient norm has to fall by at least that factor."""
    g = oracle.g
    m, _ = build("tiny_a", dtype)
    with pytest.raises(RuntimeError):
        m.logits()  # before any forward
    with torch.no_grad():
        plain_eval = run(m, g)
    own = m.logits()
    assert tuple(own.shape) == tuple(oracle.tgt.shape) + (g["t5_cfg"].vocab_size,) and own.dtype == dtype
    assert own.data_ptr() == m._engine.buffer("logits").data_ptr()  # a view
    assert rel_l2(own.float().cpu(), oracle.logits.detach()) <= 1e-4 if dtype == torch.float32 else cosine(own.float().cpu(), oracle.logits.detach()) >= 0.99
    teacher = own.clone()
    run(m, g).backward()
    plain_norm = total_norm(m)
    assert float(plain_eval) > 0 and plain_norm > 0
    m.zero_grad(set_to_none=True)
    m.set_loss_options(distill_alpha=1.0, distill_temperature=TEMP)
    loss = run(m, g, teacher)
    kl = m.token_kl().cpu()
    loss.backward()
    norm = total_norm(m)
    V = teacher.shape[-1]
    x, lab = teacher.cpu().reshape(-1, V), oracle.tgt.reshape(-1)
    dt = "f32" if dtype == torch.float32 else "bf16"
    ce = dict(LR.reference(x, lab), row_bound=torch.zeros(x.shape[0], dtype=torch.float64), gbound=torch.zeros(x.shape, dtype=torch.float64))
    r, b = DR.bounds(x.double(), x.double(), lab, dt, 0.0, 0.0, None, 1.0, TEMP, ce)
    assert bool((r["grad"] == 0).all()) and bool((r["kl_row"] == 0).all())
    factor = float(b["gbound"].norm()) / float(ce["grad"].norm())
    print(f"self-distillation {dtype}: loss {float(loss)}, max kl {float(kl.abs().max()):.3e} (bound {float(b['kl_bound'].max()):.3e}), "
          f"gradient norm {norm:.3e} against {plain_norm:.3e} plain: ratio {norm / plain_norm:.3e}, factor {factor:.3e}")
    assert bool((kl.double().abs().reshape(-1) <= b["kl_bound"]).all())
    assert abs(float(loss)) <= TEMP * TEMP * float(b["kl_bound"].max())
    assert factor < 1e-4
    assert norm <= factor * plain_norm, (norm, plain_norm, factor)


def test_grouped_labels_give_the_bits_of_the_repeated_batch(oracle):
    g = oracle.g
    inp = g["inputs"]
    tgt = inp["tgt_ids"]
    B, Lt = tgt.shape
    n, V = 2, g["t5_cfg"].vocab_size
    grouped = torch.stack([tgt, tgt.flip(0)], 1).contiguous()  # [B, n, Lt]: the second caption of an image is the other image's
    teacher = (2.0 * torch.randn(B, n, Lt, V, generator=torch.Generator().manual_seed(9))).cuda()
    w = torch.rand(B, n, Lt, generator=torch.Generator().manual_seed(10)).cuda()
    out = []
    for form in ("grouped", "repeated"):
        m, _ = build("tiny_a")
        m.set_loss_options(EPS, Z, distill_alpha=ALPHA, distill_temperature=TEMP)
        pix, src = inp["pixel_values"].cuda(), inp["src_ids"].cuda()
        if form == "grouped":
            loss = m({"pixel_values": pix}, {"input_ids": src}, {"input_ids": grouped.cuda(), "loss_weights": w, "teacher_logits": teacher})
            assert tuple(m.token_kl().shape) == (B, n, Lt)
        else:
            loss = m({"pixel_values": pix.repeat_interleave(n, 0)}, {"input_ids": src.repeat_interleave(n, 0)},
                     {"input_ids": grouped.view(B * n, Lt).cuda(), "loss_weights": w.view(B * n, Lt), "teacher_logits": teacher.view(B * n, Lt, V)})
        out.append(dict(loss=loss.detach().cpu(), tl=m.token_losses().cpu().reshape(-1), kl=m.token_kl().cpu().reshape(-1),
                        dlogits=m._engine.buffer("logits").clone().cpu()))
    for k in ("loss", "tl", "kl", "dlogits"):
        assert_equal(f"{k} (grouped against repeated)", out[0][k], out[1][k])
    assert float(out[0]["kl"].abs().max()) > 0


def test_back_to_neutral_is_the_plain_model_bit_for_bit(oracle):
    """after a distillation step, set_loss_options() and a call without a teacher issue the plain launches again: loss, per-token
    losses, d logits and every gradient that no float atomic writes equal a fresh plain model's bit for bit (the atomically written
    tensors by the project's rule: within twice the spread between plain runs, floor 2^-22 of the norm)"""
    g = oracle.g
    plains = []
    for _ in range(3):
        p, _g = build("tiny_a")
        loss = run(p, g)
        loss.backward()
        plains.append(dict(loss=loss.detach().cpu(), tl=p.token_losses().cpu(), dlogits=p._engine.buffer("logits").clone().cpu(), grads=native_grads(p)))
    p0 = plains[0]
    m, _g = build("tiny_a")
    m.set_loss_options(EPS, Z, distill_alpha=ALPHA, distill_temperature=TEMP)
    run(m, g, oracle.teachers["random"].cuda(), model_weights(g).cuda()).backward()
    assert float(m.token_kl().abs().max()) > 0
    m.zero_grad(set_to_none=True)
    m.set_loss_options()
    assert m.loss_options == {"label_smoothing": 0.0, "z_loss": 0.0}
    again = run(m, g)
    again.backward()
    with pytest.raises(RuntimeError):
        m.token_kl()  # the last loss forward had no teacher
    assert_equal("loss (back to neutral)", again.detach().cpu(), p0["loss"])
    assert_equal("token_losses (back to neutral)", m.token_losses().cpu(), p0["tl"])
    assert_equal("d logits (back to neutral)", m._engine.buffer("logits").clone().cpu(), p0["dlogits"])
    mg = native_grads(m)
    assert set(mg) == set(p0["grads"])
    dist = lambda a, b: float((a.double() - b.double()).norm())
    for k, ref in p0["grads"].items():
        if k.endswith(ATOMIC):
            spread = max(dist(plains[i]["grads"][k], plains[j]["grads"][k]) for i, j in ((0, 1), (0, 2), (1, 2)))
            assert dist(mg[k], ref) <= max(2.0 * spread, 2.0 ** -22 * float(ref.double().norm())), (k, dist(mg[k], ref), spread)
        else:
            assert_equal(f"gradient {k} (back to neutral)", mg[k], ref)


def test_bad_teachers_are_refused_and_leave_nothing_armed(oracle):
    g = oracle.g
    m, _g = build("tiny_a")
    plain = float(run(m, g))
    B, Lt = g["inputs"]["tgt_ids"].shape
    V = g["t5_cfg"].vocab_size
    good = oracle.teachers["random"].cuda()
    with pytest.raises(ValueError, match="distill_alpha is 0"):
        run(m, g, good)  # a teacher at alpha = 0
    assert float(run(m, g)) == plain
    m.set_loss_options(distill_alpha=ALPHA, distill_temperature=TEMP)
    with torch.no_grad():
        distilled = float(run(m, g, good))
    assert distilled != plain
    own = m.logits()  # (valid: the forward above wrote no gradient)
    wide = torch.zeros(B, Lt, 2 * V, device="cuda")
    bad = [(torch.zeros(B, Lt, V + 8, device="cuda"), "wrong shape"), (torch.zeros(B * Lt, V, device="cuda"), "wrong rank"),
           (oracle.teachers["random"], "wrong device"), (good.half(), "wrong dtype"), (good.double(), "wrong dtype"),
           (wide[:, :, ::2], "not contiguous"), (good.transpose(0, 1).contiguous().transpose(0, 1), "not contiguous"),
           (own, "the model's own logits"), (None, "missing at alpha > 0")]
    for t, why in bad:
        if t is not None and why == "not contiguous" and t.is_contiguous():
            continue  # (B == Lt would make the transposed form contiguous)
        with pytest.raises(ValueError) as ei:
            run(m, g, t)
        print(why, "->", str(ei.value)[:120])
        with torch.no_grad():
            assert float(run(m, g, good)) == distilled, why  # nothing stayed armed, nothing was changed
    m.set_loss_options()
    assert float(run(m, g)) == plain


def test_graph_replay_does_not_bake_the_teacher_in(oracle):
    g = oracle.g
    m, _g = build("tiny_a")
    m.use_graph = True
    m.set_loss_options(distill_alpha=ALPHA, distill_temperature=TEMP)
    order = ("random", "second", "random", "second")  # (a graph slot runs eagerly once, is captured at its second use and replayed from the third)
    teachers = {k: oracle.teachers[k].cuda() for k in set(order)}
    got = [float(run(m, g, teachers[k])) for k in order]
    want = {k: oracle.reference(k, ALPHA, TEMP)[0] for k in set(order)}
    assert abs(want["random"] - want["second"]) >= 100 * 2e-5 * abs(want["random"])  # a replayed teacher could not pass
    for k, v in zip(order, got):
        assert abs(v - want[k]) <= 2e-5 * abs(want[k]), (k, got, want)


def test_distillation_with_lora_gives_adapter_gradients_only(oracle):
    from klab_multimodalmodel_amd import lora
    g = oracle.g
    m, _g = build("tiny_a", train=False)
    ad = lora.attach(m, r=4, alpha=16, targets=("q", "v"), generator=torch.Generator().manual_seed(3))
    m.set_loss_options(distill_alpha=ALPHA, distill_temperature=TEMP)
    loss = run(m, g, oracle.teachers["random"].cuda())
    loss.backward()
    assert int(m._engine.err_view.item()) == 0 and bool(torch.isfinite(loss))
    assert float(m.token_kl().abs().max()) > 0
    grads = [p.grad for p in ad.parameters()]
    assert grads and all(gr is not None and bool(torch.isfinite(gr).all()) for gr in grads)
    assert any(float(gr.abs().max()) > 0 for gr in grads)
    assert all(p.grad is None for p in m.transformer.parameters())


def test_distillation_in_training_mode_repeats_with_the_seed(oracle):
    g = oracle.g
    teacher = oracle.teachers["random"].cuda()
    out = []
    for _ in range(2):
        torch.manual_seed(1234)
        m, _g = build("tiny_a", train=True)
        m.set_loss_options(EPS, Z, distill_alpha=ALPHA, distill_temperature=TEMP)
        w = model_weights(g).cuda()
        loss = run(m, g, teacher, w)
        tl, kl = m.token_losses().cpu().double(), m.token_kl().cpu()
        ww = w.cpu().double() * (g["inputs"]["tgt_ids"] != -100)
        assert abs(float((ww * tl).sum() / ww.sum()) - float(loss)) <= 1e-6 * abs(float(loss))
        loss.backward()
        assert int(m._engine.err_view.item()) == 0
        out.append((float(loss), kl))
    torch.manual_seed(1234)
    p, _g = build("tiny_a", train=True)
    p.set_loss_options(EPS, Z)
    plain = float(run(p, g, None, model_weights(g).cuda()))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1]) and torch.isfinite(torch.tensor(out[0][0])) and out[0][0] != plain
    assert float(out[0][1].min()) >= 0.0 and float(out[0][1].max()) > 0.0
