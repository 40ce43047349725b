"""CPU-side checks of the fused AdamW: the fixtures and bounds of tests/test_adamw_gpu.py are proved on the reference alone (an
fp32 evaluation of the kernel's sequence stays inside them), and the parts of optim.FusedAdamW / optim.decay_param_groups that
need no GPU (the torch fallback, the groups, the state dict, the constructor's errors)."""
import copy
import os
import types

import pytest
import torch

from tests import adamw_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from klab_multimodalmodel_amd.build import build_library
    build_library(verbose=False)
    from klab_multimodalmodel_amd import _lib
    return _lib.load()


# ---- the reference and its bounds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr", [2.0 ** -9, 3e-3])
@pytest.mark.parametrize("wd", [0.0, 0.01, 0.1])
def test_fp32_evaluation_of_the_sequence_stays_inside_the_bounds(wd, lr):
    """400 k elements of the fixtures' distribution through the header's sequence with every operation rounded to f32, against the
    fp64 reference: m, v within 4 * 2^-24 relative, the parameter's change within 1e-5 |dp_ref| + 3 * 2^-24 |p|.  (Measured: m 1.1,
    v 2.0 units of 2^-24; dp at most 0.65 of its bound.)"""
    h = A.one_group(wd, lr)[0]
    p, g, m, v = A.draw(A.R.gen(7), 400_000)
    m1, v1, p1 = A.adamw_f32(p, g, m, v, h)
    rm, rv, rp = A.errors(p, p1, m1, v1, A.adamw_ref(p, g, m, v, h))
    print(f"fp32 emulation wd={wd} lr={lr}: m {rm:.2f} ulp, v {rv:.2f} ulp, dp err / bound {rp:.3f}")
    assert rm <= A.M_V_ULPS and rv <= A.M_V_ULPS
    assert rp <= 1.0
    if wd <= 0.01:  # (the decay is then far smaller than the update and cannot cancel it)
        assert float((p1 - p).abs().min()) > 0  # every element moves: what the GPU test asserts for wd in {0, 0.01}


def test_zero_learning_rate_keeps_the_parameter_bits():
    h = A.group(0.0, 0.75, 1 - 2.0 ** -7, 1e-6, 0.1)
    p, g, m, v = A.draw(A.R.gen(8), 100_000)
    m1, v1, p1 = A.adamw_f32(p, g, m, v, h)
    assert torch.equal(A.bits(p1), A.bits(p))
    assert not torch.equal(m1, m) and not torch.equal(v1, v)
    assert float(A.adamw_ref(p, g, m, v, h)[2].abs().max()) == 0.0


def test_group_fixtures_are_distinct_and_every_table_uses_every_group():
    for groups in (A.three_groups(), A.sixteen_groups()):
        assert len({tuple(sorted(h.items())) for h in groups}) == len(groups)
        assert all(h["bias_corr1"] > 0 and h["bias_corr2"] > 0 for h in groups)
    assert len(A.sixteen_groups()) == A.MAX_GROUPS
    for n, ng in ((5, 3), (1100, 3), (1100, 16)):
        s = A.AdamWState(n, seed=63)
        gof = s.groups_of(ng)
        assert set(gof) == set(range(ng))
        if ng == 16:  # every group owns tensors with and without an arena copy
            assert all({s.has_a[i] for i in range(n) if gof[i] == k} == {True, False} for k in range(ng))
        else:  # the group whose learning rate is 0 has arena copies to rewrite
            assert A.three_groups()[A.ZERO_LR_GROUP]["lr"] == 0.0
            assert all(s.has_a[i] for i in range(n) if gof[i] == A.ZERO_LR_GROUP)
    assert 1100 > 1024  # the table that does not fit the kernel's LDS copy


# ---- optim.FusedAdamW without a GPU -------------------------------------------------------------------------------------------------
def _two_groups(seed):
    gen = torch.Generator().manual_seed(seed)
    ws = [torch.randn(s, generator=gen) for s in ((7, 5), (11,), (3, 4), (6,))]
    ps = [torch.nn.Parameter(w.clone()) for w in ws]
    return ps, [{"params": [ps[0], ps[2]], "weight_decay": 0.1},
                {"params": [ps[1], ps[3]], "weight_decay": 0.0, "lr": 1e-3, "betas": (0.8, 0.99), "eps": 1e-6}]


def _steps(ps, opt, n, seed=3):
    gen = torch.Generator().manual_seed(seed)
    for _ in range(n):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
        opt.zero_grad()


def test_fused_adamw_on_foreign_cpu_parameters_is_torch_adamw_bit_for_bit():
    from klab_multimodalmodel_amd.optim import FusedAdamW
    pa, ga = _two_groups(0)
    pb, gb = _two_groups(0)
    oa, ob = torch.optim.AdamW(ga, lr=3e-3), FusedAdamW(gb, lr=3e-3)
    assert [g["weight_decay"] for g in ob.param_groups] == [0.1, 0.0] and ob.param_groups[1]["betas"] == (0.8, 0.99)
    assert ob.defaults["weight_decay"] == 1e-2  # torch.optim.AdamW's default
    sched = torch.optim.lr_scheduler.LambdaLR(ob, [lambda e: 1.0, lambda e: 1.0])  # an LR scheduler accepts it
    _steps(pa, oa, 3)
    _steps(pb, ob, 3)
    assert ob._fallback is not None and ob._fb_reason == "parameters not owned by one klab MyModel"
    assert sched.get_last_lr() == [3e-3, 1e-3]
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
    assert any(not torch.equal(a.detach(), w) for a, w in zip(pa, [p.detach() for p in _two_groups(0)[0]]))


def test_state_dict_round_trips_between_fused_adamw_and_torch_adamw():
    from klab_multimodalmodel_amd.optim import FusedAdamW
    # FusedAdamW -> torch.optim.AdamW
    pa, ga = _two_groups(1)
    oa = FusedAdamW(ga, lr=2e-3)
    _steps(pa, oa, 2)
    sd = copy.deepcopy(oa.state_dict())  # (as a file would hold it: torch's load_state_dict keeps CPU tensors it is given)
    assert len(sd["param_groups"]) == 2 and sd["param_groups"][1]["betas"] == (0.8, 0.99) and sd["param_groups"][0]["weight_decay"] == 0.1
    assert all(set(st) >= {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values()) and len(sd["state"]) == 4
    pb, gb = _two_groups(1)
    ob = torch.optim.AdamW(gb, lr=9.0)  # (the loaded groups replace this learning rate)
    with torch.no_grad():
        for a, b in zip(pa, pb):
            b.copy_(a)
    ob.load_state_dict(sd)
    # torch.optim.AdamW -> FusedAdamW
    pc, gc = _two_groups(1)
    oc = FusedAdamW(gc, lr=9.0)
    with torch.no_grad():
        for a, c in zip(pa, pc):
            c.copy_(a)
    oc.load_state_dict(copy.deepcopy(ob.state_dict()))
    assert oc.param_groups[0]["lr"] == 2e-3 and oc.param_groups[1]["lr"] == 1e-3
    for ps, o in ((pa, oa), (pb, ob), (pc, oc)):
        _steps(ps, o, 2, seed=9)
    for a, b, c in zip(pa, pb, pc):
        assert torch.equal(a.detach(), b.detach()) and torch.equal(a.detach(), c.detach())


def test_a_loaded_state_with_several_step_counts_continues_in_torch():
    from klab_multimodalmodel_amd.optim import FusedAdamW
    pa, ga = _two_groups(2)
    oa = torch.optim.AdamW(ga, lr=2e-3)
    _steps(pa, oa, 2)
    sd = copy.deepcopy(oa.state_dict())
    sd["state"][1]["step"] = torch.tensor(5.0)  # one parameter joined later
    pb, gb = _two_groups(2)
    ob = FusedAdamW(gb, lr=2e-3)
    ob.load_state_dict(sd)
    assert ob._fallback is not None and ob._fb_reason == "parameters with different step counts"
    assert float(ob._fallback.state[pb[2]]["step"]) == 5.0 and float(ob._fallback.state[pb[0]]["step"]) == 2.0


def test_constructor_errors_are_torch_adamw_s():
    from klab_multimodalmodel_amd.optim import FusedAdamW
    for kw in (dict(lr=-1.0), dict(eps=-1e-8), dict(weight_decay=-0.1), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(betas=(0.9, 1.0))):
        msgs = []
        for cls in (torch.optim.AdamW, FusedAdamW):
            with pytest.raises(ValueError) as ei:
                cls([torch.nn.Parameter(torch.zeros(3))], **kw)
            msgs.append(str(ei.value))
        assert msgs[0] == msgs[1], kw
    FusedAdamW([torch.nn.Parameter(torch.zeros(3))], lr=0.0, weight_decay=0.0, betas=(0.0, 0.0), eps=0.0)


def _tiny_model(tie=True):
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    sw = SwinConfig(image_size=64, embed_dim=16, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=4)
    t5 = T5Config(vocab_size=384, d_model=128, d_kv=16, num_heads=4, d_ff=256, num_layers=2, tie_word_embeddings=tie)
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    return MyModel(args, _configs=(sw, t5, t5))


@pytest.mark.parametrize("tie", [True, False])
def test_decay_param_groups_on_a_tiny_tree(built, tie):
    from klab_multimodalmodel_amd.optim import FusedAdamW, decay_param_groups
    m = _tiny_model(tie)
    groups = decay_param_groups(m, 0.1)
    assert [g["weight_decay"] for g in groups] == [0.1, 0.0] and all(set(g) == {"params", "weight_decay"} for g in groups)
    names = {id(p): n for n, p in m.transformer.named_parameters()}
    decay, rest = ([names[id(p)] for p in g["params"]] for g in groups)
    assert rest and all(n.endswith("layer_norm.weight") or n.endswith("relative_attention_bias.weight") for n in rest)
    assert not any("layer_norm" in n or "bias" in n for n in decay)
    assert sum(n.endswith("relative_attention_bias.weight") for n in rest) == 2  # encoder and decoder, first block each
    assert sum(n.endswith("final_layer_norm.weight") for n in rest) == 2
    # the tied table once, under the name that owns it; an untied LM head decays as a matrix of its own
    assert decay.count("shared.weight") == 1 and not any("embed_tokens" in n for n in decay)
    assert ("lm_head.weight" in decay) == (not tie)
    listed = [p for g in groups for p in g["params"]]
    assert len({id(p) for p in listed}) == len(listed)
    assert {id(p) for p in listed} == {id(p) for p in m.transformer.parameters()}
    # the same through the tree, another rule, and frozen parameters are left out
    assert [[id(p) for p in g["params"]] for g in decay_param_groups(m.transformer, 0.1)] == [[id(p) for p in g["params"]] for g in groups]
    only_norms = decay_param_groups(m, 0.1, no_decay=("layer_norm",))
    assert len(only_norms[1]["params"]) == len(rest) - 2
    m.transformer.get_parameter("shared.weight").requires_grad_(False)
    assert len(decay_param_groups(m, 0.1)[0]["params"]) == len(decay) - 1
    m.transformer.get_parameter("shared.weight").requires_grad_(True)
    # torch and FusedAdamW both take the groups; on the CPU the step is torch's, and says why
    opt = FusedAdamW(groups, lr=1e-3)
    for p in m.transformer.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    assert opt._fallback is not None and opt._fb_reason == "engine not bound yet"


def test_the_library_exports_the_new_entry_points(built):
    from klab_multimodalmodel_amd import _lib, engine
    engine.lib()
    for n in ("klab_adamw_step_range", "klab_engine_adam_layout", "klab_engine_adamw_step"):
        assert hasattr(built, n) and n in (set(_lib.SIGNATURES) | set(engine.ENGINE_SIGS))
    hdr = open(os.path.join(ROOT, "include", "klab_mm.h")).read()
    assert "#define KLAB_ADAMW_MAX_GROUPS 16" in hdr and _lib.ADAMW_MAX_GROUPS == A.MAX_GROUPS == 16
    import ctypes
    assert ctypes.sizeof(_lib.AdamWGroup) == 28
    # more groups than the kernel takes (or none): refused before anything is looked at
    g = _lib.adamw_groups([A.group(1e-3, 0.9, 0.999, 1e-8, 0.0)] * 17)
    assert built.klab_adamw_step_range(None, 0, None, g, 17, 0, 0, None, None, None, None, 0, None) == _lib.ERR_UNSUPPORTED
    assert built.klab_adamw_step_range(None, 0, None, g, 0, 0, 0, None, None, None, None, 0, None) == _lib.ERR_UNSUPPORTED
    assert built.klab_adamw_step_range(None, 0, None, g, 16, 0, 0, None, None, None, None, 0, None) == _lib.ERR_BADARG
