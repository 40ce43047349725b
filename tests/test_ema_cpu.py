"""CPU-side checks of the weight EMA: the bound of tests/ema_ref.py is proved on three f32 evaluations of the rule, on the inputs
tests/test_ema_gpu.py uses, and the parts of optim.WeightEMA that need no GPU (the torch path, the decay rule, the swap, the state
dict, the guards)."""
import os

import pytest
import torch

from tests import adamw_ref as A
from tests import ema_ref as E
from tests.adamw_ref import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from klab_multimodalmodel_amd.build import build_library
    build_library(verbose=False)
    from klab_multimodalmodel_amd import _lib
    return _lib.load()


# ---- the reference and its bound ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", E.WEIGHTS)
@pytest.mark.parametrize("n", [5, 1100])
def test_three_f32_forms_stay_inside_the_bound_on_the_gpu_tests_inputs(n, w):
    """p and the shadow (the fixture's m, in the gradient layout) of AdamWState(n, 63), tensor by tensor"""
    s = A.AdamWState(n, seed=63)
    p, e = s.gather(s.p, s.poff), s.gather(s.m, s.goff)
    for name, form in E.FORMS.items():
        r = E.worst(form(p, e, w), p, e, w)
        print(f"ema n={n} w={w:.3e} {name}: err / bound {r:.3f}")
        assert r <= 1.0, (name, r)
    # most elements must move, and every f32 form moves each of those
    must = E.must_move(p, e, w)
    assert float(must.float().mean()) > 0.99
    for form in E.FORMS.values():
        assert bool((form(p, e, w)[must] != e[must]).all())


# ---- optim.WeightEMA on a small CPU module --------------------------------------------------------------------------------------------
class Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.a = torch.nn.Linear(7, 9)
        self.b = torch.nn.Linear(9, 7, bias=False)
        self.frozen = torch.nn.Parameter(torch.randn(6, generator=g), requires_grad=False)
        self.tied = torch.nn.Linear(7, 9, bias=False)
        self.tied.weight = self.a.weight
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g))


def walk(m, g):
    """what a training step does to the weights, as far as the average is concerned"""
    with torch.no_grad():
        for p in m.parameters():
            if p.requires_grad:
                p.add_(0.05 * torch.randn(p.shape, generator=g))


def tracked(m):
    return [p for _n, p in m.named_parameters() if p.requires_grad]


def shadows(ema):
    sd = ema.state_dict()["shadow"]
    return [sd[n] for n in ("a.weight", "a.bias", "b.weight")]


@pytest.mark.parametrize("warmup", [True, False])
def test_twelve_updates_follow_the_fp64_recurrence(warmup):
    from klab_multimodalmodel_amd.optim import WeightEMA
    m, g = Small(), torch.Generator().manual_seed(11)
    ema = WeightEMA(m, decay=0.5, warmup=warmup)
    e0 = [p.detach().clone() for p in tracked(m)]
    hist = []
    for t in range(1, 13):
        walk(m, g)
        ema.update()
        hist.append([p.detach().clone() for p in tracked(m)])
        want = min(0.5, (1 + t) / (10 + t)) if warmup else 0.5
        assert ema.decay_at(t) == want == E.decay_at(0.5, warmup, t)
    # the warm-up crosses over inside the 12 updates: (1 + t) / (10 + t) reaches 0.5 at t = 8
    assert E.decay_at(0.5, True, 7) == 8 / 17 < 0.5 == E.decay_at(0.5, True, 8)
    assert ema.num_updates == 12 and ema._fb_reason is not None
    for k, got in enumerate(shadows(ema)):
        ref, acc = E.recurrence([h[k] for h in hist], e0[k], 0.5, warmup)
        r = float(((got.double() - ref).abs() / acc).max())
        print(f"ema 12 updates warmup={warmup} tensor {k}: err / accumulated bound {r:.3f}")
        assert r <= 1.0
        assert got.dtype == torch.float32


def test_the_first_update_without_warmup_uses_decay():
    from klab_multimodalmodel_amd.optim import WeightEMA
    m, g = Small(), torch.Generator().manual_seed(12)
    ema = WeightEMA(m, decay=0.999, warmup=False)
    e0 = [p.detach().clone() for p in tracked(m)]
    walk(m, g)
    ema.update()
    for got, e, p in zip(shadows(ema), e0, tracked(m)):
        assert E.worst(got, p.detach(), e, E.W_999) <= 1.0
        assert E.worst(got, p.detach(), e, E.weight_at(0.999, True, 1)) > 1e3  # ... and not the warm-up's 2 / 11


def test_frozen_parameters_are_left_out_and_a_tied_one_is_tracked_once():
    from klab_multimodalmodel_amd.optim import WeightEMA
    m = Small()
    ema = WeightEMA(m)
    assert len(ema._params) == 3 and all(p.requires_grad for p in ema._params)
    assert sum(p is m.a.weight for p in ema._params) == 1
    sd = ema.state_dict()
    assert set(sd) == {"decay", "warmup", "num_updates", "shadow"}
    assert set(sd["shadow"]) == {"a.weight", "a.bias", "b.weight", "tied.weight"}  # the module's names, the alias included
    assert torch.equal(sd["shadow"]["tied.weight"], sd["shadow"]["a.weight"])
    assert (sd["decay"], sd["warmup"], sd["num_updates"]) == (0.999, True, 0)
    # a parameter iterable: the same tensor listed twice is tracked once
    it = WeightEMA([m.a.weight, m.frozen, m.a.weight, m.b.weight], decay=0.9)
    assert len(it._params) == 2 and set(it.state_dict()["shadow"]) == {"0", "2"}


@pytest.mark.parametrize("decay", [1.0, -0.1, 1.5, float("nan")])
def test_a_decay_outside_zero_one_is_refused(decay):
    from klab_multimodalmodel_amd.optim import WeightEMA
    with pytest.raises(ValueError):
        WeightEMA(Small(), decay=decay)


def test_average_parameters_swaps_in_and_back_bit_for_bit():
    from klab_multimodalmodel_amd.optim import WeightEMA
    m, g = Small(), torch.Generator().manual_seed(13)
    ema = WeightEMA(m, decay=0.5)
    for _ in range(3):
        walk(m, g)
        ema.update()
    raw = [p.detach().clone() for p in tracked(m)]
    avg = shadows(ema)
    assert not any(torch.equal(r, a) for r, a in zip(raw, avg))
    frozen = m.frozen.detach().clone()
    with ema.average_parameters() as inside:
        assert inside is ema
        assert all(torch.equal(bits(p.detach()), bits(a)) for p, a in zip(tracked(m), avg))
        assert m.tied.weight is m.a.weight
        with pytest.raises(RuntimeError, match="not re-entrant"):
            with ema.average_parameters():
                pass
        for call in (ema.update, ema.state_dict, lambda: ema.load_state_dict({})):
            with pytest.raises(RuntimeError, match="swapped in"):
                call()
        assert ema.num_updates == 3
    assert all(torch.equal(bits(p.detach()), bits(r)) for p, r in zip(tracked(m), raw))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(shadows(ema), avg))
    assert torch.equal(m.frozen, frozen)
    # the body raises: the raw weights come back all the same
    with pytest.raises(KeyError, match="body"):
        with ema.average_parameters():
            assert torch.equal(bits(m.b.weight.detach()), bits(avg[2]))
            raise KeyError("body")
    assert all(torch.equal(bits(p.detach()), bits(r)) for p, r in zip(tracked(m), raw))
    ema.update()  # ... and the average goes on
    assert ema.num_updates == 4


def test_the_state_dict_round_trip_gives_equal_bits():
    from klab_multimodalmodel_amd.optim import WeightEMA
    m, g = Small(), torch.Generator().manual_seed(14)
    ema = WeightEMA(m, decay=0.75, warmup=False)
    for _ in range(5):
        walk(m, g)
        ema.update()
    sd = ema.state_dict()
    sd["shadow"]["a.bias"][0] = 7.0  # copies: the live shadow does not follow
    assert float(ema.state_dict()["shadow"]["a.bias"][0]) != 7.0
    sd = ema.state_dict()
    fresh = WeightEMA(Small())
    fresh.load_state_dict(sd)
    assert (fresh.decay, fresh.warmup, fresh.num_updates) == (0.75, False, 5)
    back = fresh.state_dict()
    assert set(back["shadow"]) == set(sd["shadow"])
    assert all(torch.equal(bits(back["shadow"][k]), bits(sd["shadow"][k])) for k in sd["shadow"])
    m.load_state_dict(sd["shadow"], strict=False)  # the module's own names
    assert torch.equal(bits(m.b.weight.detach()), bits(sd["shadow"]["b.weight"]))
    del sd["shadow"]["b.weight"]
    with pytest.raises(KeyError, match="b.weight"):
        fresh.load_state_dict(sd)


def test_an_unbound_klab_model_takes_the_torch_path():
    import types
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    from klab_multimodalmodel_amd.optim import WeightEMA
    from tests.helpers import load_golden
    g = load_golden("tiny_a")
    sw, t5 = SwinConfig.from_dict(g["meta"]["swin_config"]), T5Config.from_dict(g["meta"]["t5_config"])
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False, transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], g["sds"]["main"]), dtype=torch.float32)
    ema = WeightEMA(m, decay=0.9)
    assert [id(p) for p in ema._params] == [id(p) for _n, p in m.transformer.named_parameters()]  # the trainable T5, not the towers
    p0 = m.transformer.get_parameter("shared.weight").detach().clone()
    with torch.no_grad():
        m.transformer.get_parameter("shared.weight").mul_(1.5)
    ema.update()
    assert ema._fb_reason == "engine not bound yet" and ema._flat is None
    sd = ema.state_dict()
    assert set(sd["shadow"]) == set(m.transformer.state_dict())  # tied aliases included
    w = E.weight_at(0.9, True, 1)
    assert E.worst(sd["shadow"]["shared.weight"], 1.5 * p0, p0, w) <= 1.0
    m.transformer.load_state_dict(sd["shadow"])


# ---- the library ----------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_new_entry_points(built):
    from klab_multimodalmodel_amd import _lib, engine
    engine.lib()
    hdr = open(os.path.join(ROOT, "include", "klab_mm.h")).read()
    for n in ("klab_ema_update_range", "klab_ema_swap_range", "klab_engine_ema_update", "klab_engine_ema_swap"):
        assert hasattr(built, n) and n in (set(_lib.SIGNATURES) | set(engine.ENGINE_SIGS))
        assert f"int {n}(" in hdr
    # refused before anything is looked at or launched: null pointers, a weight outside [0, 1], a reversed range, a foreign dtype
    one = 1 << 20  # (never dereferenced: every call below returns before a launch)
    assert built.klab_ema_update_range(None, 1, 0, 4, one, 0.5, None) == _lib.ERR_BADARG
    assert built.klab_ema_update_range(one, 1, 0, 4, None, 0.5, None) == _lib.ERR_BADARG
    assert built.klab_ema_update_range(one, 1, 0, 4, one, 1.5, None) == _lib.ERR_BADARG
    assert built.klab_ema_update_range(one, 1, 0, 4, one, -0.25, None) == _lib.ERR_BADARG
    assert built.klab_ema_update_range(one, 1, 0, 4, one, float("nan"), None) == _lib.ERR_BADARG
    assert built.klab_ema_update_range(one, 1, 4, 0, one, 0.5, None) == _lib.ERR_BADARG
    assert built.klab_ema_update_range(one, 1, -1, 4, one, 0.5, None) == _lib.ERR_BADARG
    assert built.klab_ema_update_range(one, 1, 4, 4, one, 0.5, None) == 0  # an empty range: nothing to launch
    assert built.klab_ema_swap_range(one, 1, 0, 4, one, None, _lib.BF16, None) == _lib.ERR_BADARG
    assert built.klab_ema_swap_range(one, 1, 0, 4, one, one, 77, None) == _lib.ERR_BADARG
    assert built.klab_ema_swap_range(one, 1, 4, 4, one, one, _lib.F32, None) == 0
    assert built.klab_engine_ema_update(None, one, 0.5, None) == _lib.ERR_BADARG
    assert built.klab_engine_ema_swap(None, one, None) == _lib.ERR_BADARG
