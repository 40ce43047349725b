"""optim.FusedAdafactor on the GPU: the kernels of csrc/adafactor.hip through the raw entry point on the recorded inputs of
tests/golden/adafactor.*, then the optimizer on tiny models.

The accuracy rule everywhere: the distance to the float64 result (tests/adafactor_ref.py, held to HF's float64 run by
tests/test_adafactor_cpu.py), in units of how far the optimizer moved the tensor, is at most TWICE that of an fp32 run of the
same rule in plain torch -- HF's own fp32 run from the fixture in (i), the torch fallback on the same gradients in (iii).  The
factor two covers another order of summation (the project's 2x-of-cast rule); there is no absolute constant."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import adafactor_ref as R
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

G = R.load_golden()
SETTINGS = list(G["settings"])
STATE_KEYS = ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq", "exp_avg")


# ---- (i), (ii): the raw entry point ------------------------------------------------------------------------------------------------
class Raw:
    """tensors (the fixture's unless given) behind klab_adafactor_step: separate parameters, one flat gradient buffer, an arena"""

    def __init__(self, kwargs, arena_dtype=torch.float32, shapes=None, p0=None):
        from klab_multimodalmodel_amd import _lib as L
        self.L, self.lib = L, L.load()
        self.o = dict(R.DEFAULTS, **kwargs)
        self.shapes = shapes = G["shapes"] if shapes is None else [tuple(x) for x in shapes]
        n = len(shapes)
        self.p = [torch.from_numpy(p.copy()).cuda() for p in (G["p0"] if p0 is None else p0)]
        rows = (C.c_long * n)(*[int(np.prod(s[:-1])) if len(s) >= 2 else 1 for s in shapes])
        cols = (C.c_long * n)(*[s[-1] for s in shapes])
        fact = (C.c_int * n)(*[len(s) >= 2 for s in shapes])
        out, tot = (C.c_long * (4 * n))(), (C.c_long * 4)()
        L.check(self.lib.klab_adafactor_plan(n, rows, cols, fact, out, tot), "klab_adafactor_plan")
        self.n_state, self.n_tiles, n_scratch, n_scal = list(tot)
        self.goff, desc, g = [], [], 0
        for i, s in enumerate(shapes):
            self.goff.append(g)
            aoff = g if len(s) >= 2 else -1  # like the engine: 1-D tensors have no arena copy
            desc += [self.p[i].data_ptr(), g, aoff, rows[i], cols[i], out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3], fact[i]]
            g += self.p[i].numel()
        self.soff = [out[4 * i] for i in range(n)]
        self.desc = torch.tensor(desc, dtype=torch.int64).cuda()
        self.grads = torch.zeros(g, device="cuda")
        self.state = torch.zeros(self.n_state, device="cuda")
        self.m = torch.zeros(g, device="cuda") if self.o["beta1"] is not None else None
        self.scal = torch.zeros(n_scal, device="cuda")
        self.scratch = torch.zeros(n_scratch, device="cuda")
        self.arena = torch.full((g,), 7.0, device="cuda", dtype=arena_dtype)
        self.t = 0

    def step(self, grads):
        o, L = self.o, self.L
        for i, gr in enumerate(grads):
            self.grads[self.goff[i]:self.goff[i] + gr.size] = torch.from_numpy(gr).cuda().reshape(-1)
        self.t += 1
        t = self.t
        beta2t = 1.0 - t ** o["decay_rate"]
        rel = min(1e-6 * t if o["warmup_init"] else 1e-2, 1.0 / t ** 0.5) if o["relative_step"] else o["lr"]
        L.check(self.lib.klab_adafactor_step(self.desc.data_ptr(), len(self.p), self.n_state, self.n_tiles, self.grads.data_ptr(),
                                             self.state.data_ptr(), None if self.m is None else self.m.data_ptr(), self.scal.data_ptr(),
                                             self.scratch.data_ptr(), self.arena.data_ptr(), L.dtype_code(self.arena.dtype), beta2t,
                                             1.0 - beta2t, o["eps"][0], o["eps"][1], rel, o["clip_threshold"], o["beta1"] or 0.0,
                                             1.0 - (o["beta1"] or 0.0), o["weight_decay"], int(o["scale_parameter"]), L.stream_ptr()), "klab_adafactor_step")

    def states(self, i):
        s, off = self.shapes[i], self.soff[i]
        if len(s) >= 2:
            c0 = off + ((s[0] + 3) & ~3)
            st = {"exp_avg_sq_row": self.state[off:off + s[0]], "exp_avg_sq_col": self.state[c0:c0 + s[1]]}
        else:
            st = {"exp_avg_sq": self.state[off:off + s[0]]}
        if self.m is not None:
            st["exp_avg"] = self.m[self.goff[i]:self.goff[i] + self.p[i].numel()].view(s)
        return st


@pytest.mark.parametrize("name", SETTINGS)
def test_kernels_match_float64_within_twice_hf_fp32(name):
    """(i) six steps on the fixture's tensors and gradients (every third row zero, one all-zero step)"""
    info = G["settings"][name]
    raw = Raw(info["kwargs"])
    for s in range(G["steps"]):
        raw.step(G["grads"][s])
    torch.cuda.synchronize()
    ref_p, ref_st = R.run_f64(G["p0"], G["grads"], **info["kwargs"])
    fails = []
    for i, p in enumerate(raw.p):
        assert torch.isfinite(p).all() and torch.isfinite(raw.state).all()
        err, hf = R.displacement_err(p.cpu().numpy(), ref_p[i], G["p0"][i]), info["hf_fp32_err"][i]
        print(f"{name} tensor {i} {G['shapes'][i]}: ours {err:.3e}  HF fp32 {hf:.3e}  ratio {err / hf:.2f}")
        if not err <= 2 * hf:
            fails.append((i, "p", err, hf))
        for k, v in raw.states(i).items():
            e, h = R.rel_err(v.cpu().numpy(), ref_st[i][k]), info["hf_fp32_state_err"][i][k]
            print(f"    {k}: ours {e:.3e}  HF fp32 {h:.3e}  ratio {e / h if h else float('inf'):.2f}")
            if not e <= 2 * h:
                fails.append((i, k, e, h))
        if len(G["shapes"][i]) >= 2:  # the arena copy is the new parameter
            a = raw.arena[raw.goff[i]:raw.goff[i] + p.numel()].view_as(p)
            assert torch.equal(a, p)
        # RMS(p) before the last update, as HF's state["RMS"]
        rms = float(raw.scal[4 * i + 1])
        assert abs(rms - float(G["z"][f"{name}_rms32_{i}"])) <= 1e-5 * rms
    assert not fails, fails


def test_bf16_arena_copy_and_one_dim_untouched():
    raw = Raw(G["settings"]["momentum_decay"]["kwargs"], torch.bfloat16)
    raw.step(G["grads"][0])
    torch.cuda.synchronize()
    for i, p in enumerate(raw.p):
        a = raw.arena[raw.goff[i]:raw.goff[i] + p.numel()].view_as(p)
        if len(G["shapes"][i]) >= 2:
            assert torch.equal(a, p.bfloat16())
        else:
            assert (a == 7.0).all()


@pytest.mark.parametrize("name", ["default", "momentum_decay"])
def test_step_is_bit_reproducible(name):
    """(ii) two steps from identical state and gradients give identical bits, twice over"""
    runs = []
    for _ in range(2):
        raw = Raw(G["settings"][name]["kwargs"])
        raw.step(G["grads"][0])
        raw.step(G["grads"][1])
        torch.cuda.synchronize()
        runs.append([p.clone() for p in raw.p] + [raw.state.clone(), raw.scal.clone()] + ([raw.m.clone()] if raw.m is not None else []))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- (iii) - (vii): the optimizer on tiny models -----------------------------------------------------------------------------------
def build(kind, dtype):
    if kind == "v1.0-tied":
        from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
        from klab_multimodalmodel_amd.models.model import MyModel
        g = load_golden("tiny_a")
        sw, t5 = SwinConfig.from_dict(g["meta"]["swin_config"]), T5Config.from_dict(g["meta"]["t5_config"])
        args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                     transformer_model_name="-")
        m = MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], g["sds"]["main"]), dtype=dtype)
    else:
        from tests.v11_helpers import build_v11
        m, g = build_v11("tiny_v11_a", dtype, False)
    m = m.to("cuda")
    m._direct_grads = True
    m.transformer.eval()
    return m, g


def run(m, g):
    inp = g["inputs"]
    images = {"pixel_values": inp["pixel_values"].cuda()}
    src = {"input_ids": inp["src_ids"].cuda(), "attention_mask": torch.ones_like(inp["src_ids"]).cuda()}
    tgt = {"input_ids": inp["tgt_ids"].cuda(), "attention_mask": torch.ones_like(inp["tgt_ids"]).cuda()}
    return m(images, src, tgt)


def fused_steps(m, g, opt, n, record=None):
    losses = []
    for _ in range(n):
        loss = run(m, g)
        loss.backward()
        if record is not None:
            record.append([p.grad.detach().clone() for p in m.transformer.parameters()])
        opt.step()
        opt.zero_grad()
        losses.append(float(loss))
    return losses


def replay(params, opt, grads):
    """the torch fallback: gradients that are not views of the flat buffer"""
    for gs in grads:
        for p, gr in zip(params, gs):
            p.grad = gr.clone()
        opt.step()
    for p in params:
        p.grad = None


KW = dict(beta1=0.9, weight_decay=0.01)  # relative step + parameter scale (the defaults) with momentum and decay on top


@pytest.mark.parametrize("kind", ["v1.0-tied", "v1.1-untied"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_matches_fallback_on_model(kind, dtype):
    """(iii) four eval-mode steps of the fused path; the torch fallback replays the same gradients on a twin model; the float64
    restatement replays them on the CPU.  Per tensor: fused error <= 2 x fallback error, both against float64, in displacement
    units.  (iv) the next forward's loss equals that of a fresh model loaded from state_dict(): the arena copies are current."""
    from klab_multimodalmodel_amd.optim import FusedAdafactor
    m, g = build(kind, dtype)
    twin, _ = build(kind, dtype)
    names = [n for n, _p in m.transformer.named_parameters()]
    p0 = [p.detach().cpu().numpy().copy() for p in m.transformer.parameters()]
    opt = FusedAdafactor(m.transformer.parameters(), **KW)
    rec = []
    fused_steps(m, g, opt, 4, rec)
    assert opt._flat_live and opt._fb_reason is None, opt._fb_reason  # the kernels really ran
    assert m._trainable_current()                                      # ... and the next forward skips its cast
    topt = FusedAdafactor(twin.transformer.parameters(), **KW)
    replay(list(twin.transformer.parameters()), topt, rec)
    assert topt._fb_reason is not None and not topt._flat_live
    ref, _ = R.run_f64(p0, [[x.cpu().numpy() for x in gs] for gs in rec], **KW)
    worst, fails = 0.0, []
    for n, a, b, r, z in zip(names, m.transformer.parameters(), twin.transformer.parameters(), ref, p0):
        assert torch.isfinite(a).all()
        if np.linalg.norm(r - z) == 0.0:
            assert torch.equal(a, b), n
            continue
        ea, eb = R.displacement_err(a.detach().cpu().numpy(), r, z), R.displacement_err(b.detach().cpu().numpy(), r, z)
        worst = max(worst, ea / eb)
        if not ea <= 2 * eb:
            fails.append((n, tuple(a.shape), ea, eb))
    print(f"{kind} {dtype}: worst fused / fallback error ratio over {len(names)} tensors: {worst:.3f}")
    assert not fails, fails
    # (iv) the comparison of test_fused_adam_matches_torch_adam
    nxt = float(run(m, g))
    fresh, _ = build(kind, dtype)
    fresh.load_state_dict(m.state_dict())
    want = float(run(fresh, g))
    tol = 2e-5 if dtype == torch.float32 else 2e-3
    assert abs(nxt - want) <= tol * abs(want) + 1e-6, (nxt, want)
    # an explicit write to a weight is noticed
    with torch.no_grad():
        next(m.transformer.parameters()).mul_(1.0)
    assert not m._trainable_current()


def test_step_has_no_sync():
    """(v) nothing torch can see synchronises inside step()"""
    from klab_multimodalmodel_amd.optim import FusedAdafactor
    m, g = build("v1.1-untied", torch.bfloat16)
    opt = FusedAdafactor(m.transformer.parameters(), **KW)
    fused_steps(m, g, opt, 2)
    loss = run(m, g)
    loss.backward()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert opt._flat_live and opt._steps == 3


def test_checkpoint_resume(tmp_path):
    """(vi) AsyncCheckpointer stores the whole state_dict(); the reloaded optimizer holds exactly the saved state, and 2 steps +
    save + load + 2 steps follow 4 uninterrupted steps (the comparison of test_checkpoint_resume_with_fused_adam: the
    backward's atomics make gradients differ in the last bits from run to run)"""
    from klab_multimodalmodel_amd.checkpoint import AsyncCheckpointer, load_checkpoint
    from klab_multimodalmodel_amd.optim import FusedAdafactor
    m0, g = build("v1.1-untied", torch.float32)
    ref = fused_steps(m0, g, FusedAdafactor(m0.transformer.parameters(), **KW), 4)
    m, g = build("v1.1-untied", torch.float32)
    opt = FusedAdafactor(m.transformer.parameters(), **KW)
    first = fused_steps(m, g, opt, 2)
    saved = opt.state_dict()["state"]
    ck = AsyncCheckpointer(str(tmp_path))
    path = ck.save(m, opt, step=2)
    ck.wait()
    m2, _ = build("v1.1-untied", torch.float32)
    opt2 = FusedAdafactor(m2.transformer.parameters(), **KW)
    run(m2, g)  # binds the engine
    assert load_checkpoint(path, m2, opt2) == 2
    for a, b in zip(m.transformer.parameters(), m2.transformer.parameters()):
        assert torch.equal(a, b)
    loaded = opt2.state_dict()["state"]
    assert set(loaded) == set(saved)
    for k in saved:
        assert set(saved[k]) == set(loaded[k])
        for kk in saved[k]:
            assert torch.equal(torch.as_tensor(saved[k][kk]).cpu(), torch.as_tensor(loaded[k][kk]).cpu()), (k, kk)
    rest = fused_steps(m2, g, opt2, 2)
    assert opt2._flat_live and opt2._fb_reason is None and opt2._steps == 4
    for a, b in zip(ref, first + rest):
        assert abs(a - b) <= 2e-5 * abs(a) + 1e-6, (ref, first + rest)


def test_cross_load_hf_format():
    """(vii) a state in HF's format -- written by the per-parameter rule, whose state the CPU tests hold to the fixture's schema --
    loads into the fused path, which continues like the per-parameter rule does (the 2x rule against float64)"""
    from klab_multimodalmodel_amd.optim import FusedAdafactor
    m, g = build("v1.0-tied", torch.float32)
    twin, _ = build("v1.0-tied", torch.float32)
    p0 = [p.detach().cpu().numpy().copy() for p in m.transformer.parameters()]
    rec = []
    fused_steps(m, g, FusedAdafactor(m.transformer.parameters(), **KW), 2, rec)  # only to get two steps of real gradients
    tparams = list(twin.transformer.parameters())
    topt = FusedAdafactor(tparams, **KW)
    replay(tparams, topt, rec)
    sd = topt.state_dict()
    assert set(sd["state"][0]) == {"step", "RMS", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg"}
    m2, _ = build("v1.0-tied", torch.float32)
    m2.transformer.load_state_dict(twin.transformer.state_dict())
    opt2 = FusedAdafactor(m2.transformer.parameters(), **KW)
    opt2.load_state_dict(sd)
    rec2 = []
    fused_steps(m2, g, opt2, 2, rec2)
    assert opt2._flat_live and opt2._steps == 4
    replay(tparams, topt, rec2)
    ref, _ = R.run_f64(p0, [[x.cpu().numpy() for x in gs] for gs in rec + rec2], **KW)
    fails = []
    for a, b, r, z in zip(m2.transformer.parameters(), tparams, ref, p0):
        if np.linalg.norm(r - z) == 0.0:
            continue
        ea, eb = R.displacement_err(a.detach().cpu().numpy(), r, z), R.displacement_err(b.detach().cpu().numpy(), r, z)
        if not ea <= 2 * eb:
            fails.append((tuple(a.shape), ea, eb))
    assert not fails, fails
    # and back: the fused state in HF's keys
    back = opt2.state_dict()["state"]
    assert set(back[0]) == set(sd["state"][0]) and back[0]["step"] == 4
