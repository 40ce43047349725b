"""What tests/test_distill_gpu.py takes for granted, proved without a GPU: the fp64 reference of tests/distill_ref.py is
torch.nn.functional.cross_entropy plus kl_div(log_target=True) put together in fp64, its gradient is autograd's, at alpha = 0 it is
loss_opts_ref.reference; the bounds are finite, positive on scored rows and zero elsewhere; MyModel.set_loss_options validates and
reads the distillation options back; the C ABI declares the two new entry points."""
import math
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from tests import distill_ref as DR
from tests import loss_opts_ref as LR
from tests.helpers import load_golden
from tests.rowops_ref import ce_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(6, 2056, "bf16", "bf16"), (6, 1028, "f32", "f32"), (261, 1028, "f32", "f32"), (6, 2056, "bf16", "f32")]


def close(a, b, rel=1e-12):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    scale = float(b.abs().max()) if b.numel() else 0.0
    return float((a - b).abs().max()) <= rel * max(scale, 1e-300)


@pytest.mark.parametrize("rows,V,dt,tdt", CASES)
@pytest.mark.parametrize("alpha,T", DR.SETTINGS)
def test_reference_is_cross_entropy_plus_kl_div(rows, V, dt, tdt, alpha, T):
    c = ce_case(rows, V, dt)
    t = DR.teacher_for(rows, V, dt, tdt).double()
    assert bool(torch.isfinite(t).all())
    x = c["stored"].double()
    valid = c["valid"]
    n = int(valid.sum())
    ce = F.cross_entropy(x, c["labels"], ignore_index=-100)
    kl = F.kl_div(torch.log_softmax(x / T, -1), torch.log_softmax(t / T, -1), reduction="none", log_target=True).sum(-1)
    want = (1.0 - alpha) * ce + alpha * T * T * kl[valid].sum() / n
    r = DR.reference(c["stored"], t, c["labels"], alpha=alpha, T=T)
    assert close(r["loss"], want), (r["loss"], float(want))
    assert close(r["kl_row"][valid], kl[valid], 1e-10) and bool((r["kl_row"][~valid] == 0).all())
    assert bool((r["kl_row"][valid] > 0).all())


@pytest.mark.parametrize("rows,V,dt,tdt", CASES)
@pytest.mark.parametrize("alpha,T", DR.SETTINGS)
@pytest.mark.parametrize("eps,z", DR.OPTIONS)
@pytest.mark.parametrize("weighted", [False, True])
def test_reference_gradient_is_autograd(rows, V, dt, tdt, alpha, T, eps, z, weighted):
    c = ce_case(rows, V, dt)
    t = DR.teacher_for(rows, V, dt, tdt)
    w = LR.weights_for(rows, V) if weighted else None
    x = c["stored"].double().clone().requires_grad_(True)
    want = DR.torch_loss(x, t, c["labels"], eps, z, w, alpha, T)
    (gw,) = torch.autograd.grad(want, x)
    r = DR.reference(c["stored"], t, c["labels"], eps, z, w, alpha, T)
    assert close(r["loss"], want.detach()) and close(r["grad"], gw, 1e-11)
    assert bool((r["grad"][~c["valid"]] == 0).all()) and bool((r["loss_row"][~c["valid"]] == 0).all())
    if weighted:
        dead = c["valid"] & (w == 0)
        assert bool(dead.any()) and bool((r["grad"][dead] == 0).all()) and bool((r["loss_row"][dead] != 0).all())


@pytest.mark.parametrize("rows,V,dt,tdt", CASES)
@pytest.mark.parametrize("eps,z", DR.OPTIONS)
def test_alpha_zero_is_the_options_reference(rows, V, dt, tdt, eps, z):
    c = ce_case(rows, V, dt)
    w = LR.weights_for(rows, V)
    want = LR.reference(c["stored"], c["labels"], eps, z, w)
    for T in (1.0, 2.0):
        r = DR.reference(c["stored"], DR.teacher_for(rows, V, dt, tdt), c["labels"], eps, z, w, alpha=0.0, T=T)
        assert r["loss"] == want["loss"] and torch.equal(r["loss_row"], want["loss_row"]) and torch.equal(r["grad"], want["grad"])


@pytest.mark.parametrize("rows,V,dt,tdt", CASES + [(6, 8, "bf16", "bf16"), (6, 4, "f32", "f32"), (6, 40000, "bf16", "f32")])
@pytest.mark.parametrize("alpha,T", DR.SETTINGS)
@pytest.mark.parametrize("same", [False, True])
def test_bounds_are_finite_positive_on_scored_rows_and_zero_elsewhere(rows, V, dt, tdt, alpha, T, same):
    assert DR.FACTOR == 1.0
    for eps, z in DR.OPTIONS:
        for weighted in (False, True):
            c = DR.distill_case(rows, V, dt, tdt, eps, z, weighted, alpha, T, same)
            v = c["valid"]
            for k in ("kl_bound", "row_bound", "gbound", "loss_bound"):
                assert bool(torch.isfinite(c[k]).all()), k
            for k in ("kl_bound", "row_bound"):
                assert bool((c[k][v] > 0).all()) and bool((c[k][~v] == 0).all()), k
            live = v if c["weights"] is None else v & (c["weights"] > 0)
            assert bool(live.any()) and bool((c["gbound"][live] > 0).all()) and bool((c["gbound"][~live] == 0).all())
            # bounds that are no tolerances in disguise: far below the values they guard
            # (2e-4: the two-pass form's worst-case chain of 22 rescalings at V = 40000 alone is 1e-4 of a loss of 3)
            assert float(c["loss_bound"]) < 2e-4 * abs(float(c["loss"])) or same
            assert bool((c["kl_bound"] <= 1e-4 * (1.0 + c["kl_row"].abs())).all())  # (kl reaches hundreds: the +-150 / -200 logits)
            assert bool((c["row_bound"] <= 1e-4 * max(1.0, alpha * T * T) * (1.0 + c["loss_row"].abs())).all())
            if same:
                assert bool((c["kl_row"] == 0).all())
                if alpha == 1.0:
                    assert bool((c["grad"] == 0).all())


def tiny_model():
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_golden("tiny_a")
    sw, t5 = SwinConfig.from_dict(g["meta"]["swin_config"]), T5Config.from_dict(g["meta"]["t5_config"])
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    return MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], g["sds"]["main"]), dtype=torch.float32)


def test_set_loss_options_validates_and_reads_the_distillation_options_back():
    m = tiny_model()
    assert m.loss_options == {"label_smoothing": 0.0, "z_loss": 0.0}
    m.set_loss_options(0.1, 1e-4)  # the two-argument call behaves as before
    assert m.loss_options == {"label_smoothing": 0.1, "z_loss": 1e-4}
    m.set_loss_options(0.1, 1e-4, distill_alpha=0.5, distill_temperature=2.0)
    full = {"label_smoothing": 0.1, "z_loss": 1e-4, "distill_alpha": 0.5, "distill_temperature": 2.0}
    assert m.loss_options == full
    for kw in (dict(distill_alpha=-0.1), dict(distill_alpha=1.5), dict(distill_alpha=math.nan), dict(distill_alpha=math.inf),
               dict(distill_alpha=0.5, distill_temperature=0.0), dict(distill_alpha=0.5, distill_temperature=-1.0),
               dict(distill_temperature=math.inf), dict(distill_temperature=math.nan), dict(label_smoothing=1.0, distill_alpha=0.5)):
        with pytest.raises(ValueError) as ei:
            m.set_loss_options(**kw)
        assert "has to be" in str(ei.value)
        assert m.loss_options == full  # a refused call changes nothing
    m.set_loss_options(distill_alpha=1.0)
    assert m.loss_options == {"label_smoothing": 0.0, "z_loss": 0.0, "distill_alpha": 1.0, "distill_temperature": 1.0}
    m.set_loss_options()
    assert m.loss_options == {"label_smoothing": 0.0, "z_loss": 0.0}
    assert not any("distill" in k or "loss" in k for k in m.state_dict())
    for fn in (m.token_kl, m.logits):
        with pytest.raises(RuntimeError):
            fn()


def test_entry_points_are_declared():
    from klab_multimodalmodel_amd import _lib, distill, ops
    hdr = open(os.path.join(ROOT, "include", "klab_mm.h")).read()
    for name, nargs in (("klab_ce_fwd_distill", 20), ("klab_engine_set_distill", 5)):
        mt = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert mt, f"{name} is not declared in include/klab_mm.h"
        assert len(mt.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(_lib.load(), name), f"{name} is not exported by the built library"
    assert callable(ops.ce_fwd_distill) and callable(distill.teacher_logits)
