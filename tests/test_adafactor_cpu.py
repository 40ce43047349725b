"""optim.FusedAdafactor without a GPU: the float64 restatement and the torch fallback against the recorded run of
transformers.optimization.Adafactor (tests/golden/adafactor.*), the constructor, the state-dict schema, the C ABI."""
import copy

import numpy as np
import pytest
import torch

from tests import adafactor_ref as R

G = R.load_golden()
SETTINGS = list(G["settings"])
STATE_KEYS = ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq", "exp_avg")
EPS64 = float(np.finfo(np.float64).eps)


def make_opt(name, dtype=torch.float32):
    from klab_multimodalmodel_amd.optim import FusedAdafactor
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(dtype)) for p in G["p0"]]
    return ps, FusedAdafactor(ps, **G["settings"][name]["kwargs"])


def run_steps(ps, opt, steps):
    for s in steps:
        for p, g in zip(ps, G["grads"][s]):
            p.grad = torch.from_numpy(g.copy()).to(p.dtype)
        opt.step()


@pytest.mark.parametrize("name", SETTINGS)
def test_restatement_matches_hf_float64(name):
    """tests/adafactor_ref.py is the rule: HF's float64 run, on the stored rows, up to float64 rounding.  Both sides round every
    intermediate of six steps to 2^-53 relative; what reaches p is a few ulps of p per step, so the bound in displacement units
    is 64 eps ||p|| / ||p - p0|| (plus 1e-12 for the chain of roundings inside u itself)."""
    ps, sts = R.run_f64(G["p0"], G["grads"], **G["settings"][name]["kwargs"])
    for i, p in enumerate(ps):
        rows = G["rows"](i)
        ref = G["z"][f"{name}_p64_{i}"]
        assert np.isfinite(p).all()
        bound = 1e-12 + 64 * EPS64 * np.linalg.norm(ref) / np.linalg.norm(ref - G["p0"][i][rows].astype(np.float64))
        err = R.displacement_err(p[rows], ref, G["p0"][i][rows])
        print(name, i, "restatement vs HF f64:", err, "bound", bound)
        assert err <= bound
        for k in STATE_KEYS:
            if f"{name}_{k}64_{i}" in G["z"].files:
                sub = rows if k == "exp_avg" else slice(None)
                assert R.rel_err(sts[i][k][sub], G["z"][f"{name}_{k}64_{i}"]) <= 1e-12, (name, i, k)
            else:
                assert k not in sts[i]


@pytest.mark.parametrize("name", SETTINGS)
def test_fallback_matches_hf_fp32(name):
    """plain parameters -> the per-parameter torch rule inside optim.py.  In fp32 on the CPU it is held to the project's
    2x rule with HF's own fp32 run as the yardstick: its distance to the float64 result, in displacement units, is at most
    twice HF's.  In float64 it reproduces HF's float64 run."""
    ps, opt = make_opt(name)
    run_steps(ps, opt, range(G["steps"]))
    assert opt._fb_reason is not None and not opt._flat_live
    for i, p in enumerate(ps):
        rows = G["rows"](i)
        p0, p64, p32 = G["p0"][i][rows], G["z"][f"{name}_p64_{i}"], G["z"][f"{name}_p32_{i}"]
        assert torch.isfinite(p).all()
        ours, hf = R.displacement_err(p.detach().numpy()[rows], p64, p0), R.displacement_err(p32, p64, p0)
        print(name, i, "fallback fp32:", ours, "HF fp32:", hf)
        assert ours <= 2 * hf
        st = opt.state[p]
        assert st["step"] == G["steps"]
        for k in STATE_KEYS:
            if f"{name}_{k}64_{i}" in G["z"].files:
                sub = rows if k == "exp_avg" else slice(None)
                ref64 = G["z"][f"{name}_{k}64_{i}"]
                assert R.rel_err(st[k].numpy()[sub], ref64) <= 2 * R.rel_err(G["z"][f"{name}_{k}32_{i}"], ref64), (name, i, k)
            else:
                assert k not in st
    ps, opt = make_opt(name, torch.float64)
    run_steps(ps, opt, range(G["steps"]))
    for i, p in enumerate(ps):
        rows = G["rows"](i)
        ref = G["z"][f"{name}_p64_{i}"]
        bound = 1e-12 + 64 * EPS64 * np.linalg.norm(ref) / np.linalg.norm(ref - G["p0"][i][rows].astype(np.float64))
        assert R.displacement_err(p.detach().numpy()[rows], ref, G["p0"][i][rows]) <= bound


def test_constructor_errors():
    from klab_multimodalmodel_amd.optim import FusedAdafactor
    p = [torch.nn.Parameter(torch.zeros(4, 4))]
    with pytest.raises(ValueError, match="Cannot combine manual `lr` and `relative_step=True` options"):
        FusedAdafactor(p, lr=1e-3)
    with pytest.raises(ValueError, match="`warmup_init=True` requires `relative_step=True`"):
        FusedAdafactor(p, lr=1e-3, relative_step=False, warmup_init=True)
    opt = FusedAdafactor(p)
    assert opt.defaults == dict(lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0.0,
                                scale_parameter=True, relative_step=True, warmup_init=False)


@pytest.mark.parametrize("name", SETTINGS)
def test_state_dict_schema_and_round_trip(name):
    """per-parameter keys are the fixture's (HF's); a saved state loads into a fresh optimizer, which continues identically"""
    ps, opt = make_opt(name)
    run_steps(ps, opt, range(3))
    sd = copy.deepcopy(opt.state_dict())
    assert sorted(sd["state"]) == list(range(len(ps)))
    for i in range(len(ps)):
        want = {"step", "RMS"} | {k for k in STATE_KEYS if f"{name}_{k}64_{i}" in G["z"].files}
        assert set(sd["state"][i]) == want
        assert sd["state"][i]["step"] == 3
    assert set(sd["param_groups"][0]) >= set(opt.defaults) | {"params"}
    ps2, opt2 = make_opt(name)
    with torch.no_grad():
        for a, b in zip(ps2, ps):
            a.copy_(b)
    opt2.load_state_dict(sd)
    run_steps(ps, opt, range(3, G["steps"]))
    run_steps(ps2, opt2, range(3, G["steps"]))
    for a, b in zip(ps, ps2):
        assert torch.equal(a, b)
    assert opt2.state[ps2[0]]["step"] == G["steps"]


def test_foreign_parameters_and_groups_take_the_fallback():
    from klab_multimodalmodel_amd.optim import FusedAdafactor
    a, b = torch.nn.Parameter(torch.randn(8, 12)), torch.nn.Parameter(torch.randn(12))
    opt = FusedAdafactor([{"params": [a]}, {"params": [b], "weight_decay": 0.1}], lr=1e-2, relative_step=False)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.5 ** e)
    before = [a.detach().clone(), b.detach().clone()]
    for _ in range(2):
        a.grad, b.grad = torch.randn_like(a), torch.randn_like(b)
        loss = opt.step(lambda: torch.tensor(3.0))
        assert float(loss) == 3.0
        sched.step()
        opt.zero_grad()
    assert opt._fb_reason == "several param groups" and not opt._flat_live
    assert opt.param_groups[0]["lr"] == pytest.approx(0.25e-2)
    assert not torch.equal(a, before[0]) and not torch.equal(b, before[1])
    assert a.grad is None and opt.state[b]["step"] == 2 and "exp_avg_sq" in opt.state[b] and "exp_avg_sq_row" in opt.state[a]


def test_c_abi_symbols():
    from klab_multimodalmodel_amd import _lib, engine
    lib = _lib.load()
    for n in ("klab_adafactor_plan", "klab_adafactor_step"):
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    for n in ("klab_engine_adafactor_state_elems", "klab_engine_adafactor_step", "klab_engine_adafactor_layout"):
        assert n in engine.ENGINE_SIGS and hasattr(lib, n)


def test_plan_layout():
    """the host planner behind both entry points: offsets are 16-byte aligned, tiles cover every row once, scratch holds it all"""
    import ctypes as C

    from klab_multimodalmodel_amd import _lib
    lib = _lib.load()
    shapes = [(32128, 512), (512, 2048), (32, 6), (512,), (384, 512), (512, 384)]
    n = len(shapes)
    rows = (C.c_long * n)(*[s[0] if len(s) == 2 else 1 for s in shapes])
    cols = (C.c_long * n)(*[s[-1] for s in shapes])
    fact = (C.c_int * n)(*[len(s) == 2 for s in shapes])
    out, tot = (C.c_long * (4 * n))(), (C.c_long * 4)()
    assert lib.klab_adafactor_plan(n, rows, cols, fact, out, tot) == 0
    soff = tile = part = 0
    for i, s in enumerate(shapes):
        o, t0, tl, po = out[4 * i:4 * i + 4]
        assert (o, t0) == (soff, tile) and o % 4 == 0 and tl % 4 == 0
        if len(s) == 2:
            ntl = -(-s[0] // tl)
            assert po == part and ntl <= 128 and tl <= 512
            soff += -(-s[0] // 4) * 4 + -(-s[1] // 4) * 4
            part += ntl * s[1]
        else:
            ntl = -(-s[0] // tl)
            soff += s[0]
        tile += ntl
    assert list(tot) == [soff, tile, soff + 4 * tile + part, 4 * n]
    bad_rows, bad_cols, one = (C.c_long * 1)(3), (C.c_long * 1)(5), (C.c_int * 1)(1)
    assert lib.klab_adafactor_plan(1, bad_rows, bad_cols, one, out, tot) == _lib.ERR_UNSUPPORTED  # 15 elements: not a multiple of 4
