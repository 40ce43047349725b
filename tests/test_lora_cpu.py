"""CPU-side checks of the LoRA adapters: the bounds of tests/lora_ref.py are proved on three f32 evaluation orders, on the inputs
tests/test_lora_kernels_gpu.py uses; the integer fixtures are shown to be exact in f32 (and, merged, in bf16); the must-move share of
the randn fixtures is counted; and the host logic of klab_multimodalmodel_amd.lora that needs no GPU (target selection, names, init,
guards, state dict)."""
import types

import pytest
import torch

from tests import lora_ref as R
from tests.adamw_ref import bits

DTYPES = (torch.bfloat16, torch.float32)


# ---- the references and their bounds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", R.RANKS)
def test_three_f32_orders_stay_inside_the_bounds_on_the_gpu_tests_inputs(r):
    f = R.Fixture(7, r, "randn")
    for order in R.ORDERS:
        wm = wa = wb = 0.0
        for W, A, B, dW in zip(f.W, f.A, f.B, f.dW):
            for dt in DTYPES:
                exact, bound = R.merge_ref(W, A, B, f.s, dt)
                wm = max(wm, R.worst(R.merge_f32(W, A, B, f.s, order, dt), exact, bound))
            dA, bA, dB, bB = R.grads_ref(dW, A, B, f.s)
            gA, gB = R.grads_f32(dW, A, B, f.s, order)
            wa, wb = max(wa, R.worst(gA, dA, bA)), max(wb, R.worst(gB, dB, bB))
        print(f"lora r={r} {order}: err / bound merge {wm:.3f} dA {wa:.3f} dB {wb:.3f}")
        assert wm <= 1.0 and wa <= 1.0 and wb <= 1.0, (order, wm, wa, wb)


@pytest.mark.parametrize("r", R.RANKS)
@pytest.mark.parametrize("n", R.NTAB)
def test_integer_fixtures_are_exact_in_f32_in_any_order(n, r):
    f = R.Fixture(n, r, "int")
    assert f.s == 0.5
    for W, A, B, dW in zip(f.W, f.A, f.B, f.dW):
        # every partial sum of integer products is an integer below 2^24 in magnitude, whatever the order; s is a power of two
        assert float(W.abs().max() + (B.abs() @ A.abs()).max()) < 2 ** 24
        assert float((B.abs().t() @ dW.abs()).max()) < 2 ** 24 and float((dW.abs() @ A.abs().t()).max()) < 2 ** 24
        for t in (W, A, B, dW):
            assert torch.equal(t, t.round())
        exact = R.merge_ref(W, A, B, f.s, torch.float32)[0]
        dA, _ba, dB, _bb = R.grads_ref(dW, A, B, f.s)
        assert torch.equal(exact.to(torch.bfloat16).double(), exact)  # the merged value fits the 8 bits of bf16
        for order in R.ORDERS:
            for dt in DTYPES:
                assert torch.equal(R.merge_f32(W, A, B, f.s, order, dt).double(), exact), (order, dt)
            gA, gB = R.grads_f32(dW, A, B, f.s, order)
            assert torch.equal(gA.double(), dA) and torch.equal(gB.double(), dB), order


@pytest.mark.parametrize("r", R.RANKS)
@pytest.mark.parametrize("n", R.NTAB)
def test_randn_fixtures_move_at_least_99_percent_of_the_elements(n, r):
    f = R.Fixture(n, r, "randn")
    for dt in DTYPES:
        must = torch.cat([R.must_move(W, A, B, f.s, dt).reshape(-1) for W, A, B in zip(f.W, f.A, f.B)])
        share = float(must.float().mean())
        print(f"lora n={n} r={r} {dt}: must-move share {share:.4f}")
        assert share >= 0.99
        for W, A, B in zip(f.W, f.A, f.B):  # and a correct f32 evaluation moves each of them
            mv = R.must_move(W, A, B, f.s, dt)
            assert bool((R.merge_f32(W, A, B, f.s, "forward", dt)[mv] != W.to(dt)[mv]).all())


def test_fixture_layouts_do_not_overlap_and_b_zero_is_zero():
    f = R.Fixture(7, 8, "randn", b_zero=True)
    assert all(float(b.abs().max()) == 0.0 for b in f.B)
    m = f.arena_mask()
    assert int(m.sum()) == sum(o * i for o, i in f.shapes) and not bool(m[f.other:f.other + 256].any())
    assert len({s for s in f.shapes}) == 3 and all(a % 4 == 0 for a in f.aoff + f.goff)
    g = f.grads()
    for d, go in zip(f.dW, f.goff):
        assert torch.equal(g[go:go + d.numel()].view(d.shape), d)


# ---- host logic --------------------------------------------------------------------------------------------------------------------------
def tiny(v11=False, dtype="fp32"):
    from klab_multimodalmodel_amd.build import build_library
    build_library(verbose=False)
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    sw = SwinConfig(image_size=56, embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=7)
    kw = dict(feed_forward_proj="gated-gelu", tie_word_embeddings=False, scale_decoder_outputs=False) if v11 else {}
    t5 = T5Config(vocab_size=512, d_model=64, d_kv=32, num_heads=2, d_ff=128, num_layers=2, **kw)
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    return MyModel(args, _configs=(sw, t5, t5), _seed=1, dtype=dtype)


@pytest.fixture(scope="module")
def names():
    return {v: [n for n, _p in tiny(v11=v).transformer.named_parameters()] for v in (False, True)}


def test_target_selection_on_v10_and_v11_parameter_lists(names):
    from klab_multimodalmodel_amd import lora
    v10, v11 = names[False], names[True]
    t, mods = lora.select_targets(v10, ("v", "q"))
    assert t == ("q", "v")
    # every block and every attention kind: 2 encoder self + 2 decoder self + 2 cross, q and v each
    assert len(mods) == 12 and "decoder.block.1.layer.1.EncDecAttention.v" in mods and "encoder.block.0.layer.0.SelfAttention.q" in mods
    t, mods = lora.select_targets(v10, "all-linear")
    assert t == ("q", "k", "v", "o", "wi", "wo") and len(mods) == 6 * 4 + 4 * 2
    t, mods = lora.select_targets(v11, "all-linear")
    assert t == ("q", "k", "v", "o", "wi_0", "wi_1", "wo") and len(mods) == 6 * 4 + 4 * 3
    assert lora.select_targets(v11, "wi_0")[1] == [m for m in mods if m.endswith(".wi_0")]
    for nm in (v10, v11):
        for m in lora.select_targets(nm, "all-linear")[1]:  # never adapted
            assert not any(x in m for x in ("shared", "lm_head", "layer_norm", "relative_attention_bias", "embed_tokens"))
    for bad, nm in ((("q", "lm_head"), v11), (("shared",), v10), (("wi",), v11), (("wi_0",), v10), ((), v10), ("dense", v10)):
        with pytest.raises(ValueError):
            lora.select_targets(nm, bad)


def test_attach_names_init_and_seed():
    from klab_multimodalmodel_amd import lora
    m = tiny()
    flags = {n: p.requires_grad for n, p in m.transformer.named_parameters()}
    assert all(flags.values())
    ad = lora.attach(m, r=4, alpha=16, targets=("q", "v"), generator=torch.Generator().manual_seed(3))
    assert not any(p.requires_grad for p in m.transformer.parameters())
    named = dict(ad.named_parameters())
    assert "encoder.block.0.layer.0.SelfAttention.q.lora_A.weight" in named and "decoder.block.1.layer.1.EncDecAttention.v.lora_B.weight" in named
    assert len(named) == 24 and [id(p) for p in ad.parameters()] == [id(p) for p in named.values()]
    for k, p in named.items():
        w = m.transformer.get_parameter(k.rsplit(".lora_", 1)[0] + ".weight")
        assert p.requires_grad and p.dtype == torch.float32
        if ".lora_A." in k:
            assert tuple(p.shape) == (4, w.shape[1])
            top = float(p.detach().abs().max())
            assert 0.5 * w.shape[1] ** -0.5 < top <= w.shape[1] ** -0.5
        else:
            assert tuple(p.shape) == (w.shape[0], 4) and float(p.detach().abs().max()) == 0.0
    assert ad.scale == 4.0
    sd = ad.state_dict()
    assert sd["r"] == 4 and sd["alpha"] == 16.0 and sd["targets"] == ("q", "v") and set(sd) == set(named) | {"r", "alpha", "targets"}
    with pytest.raises(RuntimeError):
        lora.attach(m, r=4)  # already has adapters
    ad.detach()
    assert {n: p.requires_grad for n, p in m.transformer.named_parameters()} == flags and m._lora is None
    with pytest.raises(RuntimeError):
        ad.detach()
    # the same generator seed gives the same bits, the global generator serves when none is given
    ad2 = lora.attach(m, r=4, alpha=16, targets=("q", "v"), generator=torch.Generator().manual_seed(3))
    assert all(torch.equal(bits(a.detach()), bits(b)) for a, b in zip(ad2.parameters(), named.values()))
    ad2.detach()
    torch.manual_seed(9)
    a1 = [p.detach().clone() for p in lora.attach(m, r=2).parameters()]
    m._lora.detach()
    torch.manual_seed(9)
    a2 = [p.detach().clone() for p in lora.attach(m, r=2).parameters()]
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(a1, a2))
    # recorded flags come back as they were, not as all-True
    m._lora.detach()
    m.transformer.get_parameter("shared.weight").requires_grad_(False)
    ad3 = lora.attach(m, r=2)
    ad3.detach()
    assert not m.transformer.get_parameter("shared.weight").requires_grad
    assert m.transformer.get_parameter("encoder.block.0.layer.0.SelfAttention.q.weight").requires_grad


def test_attach_refuses_what_it_cannot_do():
    from klab_multimodalmodel_amd import lora
    from klab_multimodalmodel_amd.ddp import DistributedDataParallel
    m = tiny()
    for bad in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError):
            lora.attach(m, r=bad)
    for bad in (0, -1.0, float("nan"), float("inf"), "16"):
        with pytest.raises(ValueError):
            lora.attach(m, alpha=bad)
    with pytest.raises(ValueError):
        lora.attach(m, targets=("q", "dense"))
    with pytest.raises(ValueError):
        lora.attach(m, targets=("wi_0",))  # a v1.0 model has no gated feed-forward
    assert m._lora is None and all(p.requires_grad for p in m.transformer.parameters())  # a refused attach changes nothing
    with pytest.raises(NotImplementedError):
        lora.attach(tiny(dtype="fp8"))
    ad = lora.attach(m, r=2)
    with pytest.raises(NotImplementedError):
        DistributedDataParallel(m)  # wrapping a model with adapters
    assert m._reducer is None and m._segment_hook is None
    ad.detach()
    ddp = DistributedDataParallel(m)
    with pytest.raises(NotImplementedError):
        lora.attach(ddp)  # attaching to the wrapper ...
    with pytest.raises(NotImplementedError):
        lora.attach(m)    # ... or to the wrapped model
    assert m._lora is None


def test_state_dict_round_trip_and_its_checks(tmp_path):
    from klab_multimodalmodel_amd import lora
    m = tiny()
    ad = lora.attach(m, r=3, alpha=6, targets=("q", "wo"), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        for p in ad.parameters():
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())))
    want = {k: v.clone() for k, v in ad.state_dict().items() if torch.is_tensor(v)}
    path = str(tmp_path / "style_a.pt")
    ad.save(path)
    ad.detach()
    ad = lora.attach(m, r=3, alpha=6, targets=("wo", "q"))
    assert not all(torch.equal(p.detach(), want[k]) for k, p in ad.named_parameters())
    v0 = [p._version for p in ad.parameters()]
    ad.load(path)
    assert all(torch.equal(bits(p.detach()), bits(want[k])) for k, p in ad.named_parameters())
    assert all(p._version > v for p, v in zip(ad.parameters(), v0))  # load writes in place: the version counters move
    sd = ad.state_dict()
    for key, val in (("r", 4), ("alpha", 12.0), ("targets", ("q",))):
        with pytest.raises(ValueError):
            ad.load_state_dict({**sd, key: val})
    k0 = next(iter(want))
    with pytest.raises(ValueError):
        ad.load_state_dict({**sd, k0: torch.zeros(5, 5)})
    with pytest.raises(ValueError):
        ad.load_state_dict({k: v for k, v in sd.items() if k != k0})
    with pytest.raises(ValueError):
        ad.load_state_dict({**sd, "encoder.block.9.layer.0.SelfAttention.q.lora_A.weight": torch.zeros(3, 64)})
    with pytest.raises(ValueError):
        ad.load_state_dict({k: v for k, v in sd.items() if k != "alpha"})
    assert all(torch.equal(bits(p.detach()), bits(want[k])) for k, p in ad.named_parameters())  # a refused load changes nothing


def test_plan_of_the_device_table():
    from klab_multimodalmodel_amd import ops
    rb = ops.lora_row_block()
    assert rb == 64  # (tests/lora_ref.SHAPES end in partial row blocks of this height)
    assert sum(o > 2 * rb and o % rb != 0 for o, _i in R.SHAPES) >= 2  # three row blocks or more, the last one partial
    plan, n_out, n_slab = ops.lora_plan([(64, 64, 8), (136, 200, 3), (520, 72, 3)])
    assert plan[0] == (0, 0, 0, 4 * (128 + 150 + 54))
    assert plan[1][:3] == (128, 1, 8 * 64) and plan[2][:3] == (128 + 150, 1 + 3, 8 * 64 + 3 * 3 * 200)
    assert plan[1][3] == plan[0][3] + 64 * 8 and plan[2][3] == plan[1][3] + 136 * 3
    assert n_out == plan[2][3] + 520 * 3 and n_slab == 8 * 64 + 9 * 200 + 9 * 3 * 72
    for bad in ((64, 66, 8), (64, 64, 0), (64, 64, 65), (0, 64, 4)):
        with pytest.raises(ValueError):
            ops.lora_plan([bad])
