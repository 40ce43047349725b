"""Writes tests/golden/adafactor.npz / adafactor.json: six steps of `transformers.optimization.Adafactor` on CPU.

    python tests/golden/make_adafactor_goldens.py

Four tensors -- (1024, 64), (64, 256), (32, 8), (64,) -- under four settings.  The gradients are recorded; every third row of a
2-D gradient is exactly zero (embedding rows no token hit) and step 3 (of 0..5) has an all-zero gradient.  Each setting is run
twice from the same initial parameters: in fp32 (what a user of HF gets) and in float64 (the rule itself).  The json holds, per
setting and tensor, HF's own fp32 error  ||p_fp32 - p_f64|| / ||p_f64 - p_0||  after the six steps OVER THE WHOLE TENSOR (and the
same for every state tensor, relative to the state's own norm): the yardstick of tests/test_adafactor_gpu.py.

To stay under 1 MiB the inputs are stored as int8 (`k`) with a power-of-two scale in the json -- value = float32(k) * 2**-e,
exact in fp32 and in float64 -- and of the two large tensors' final parameters and first moments only every ROW_STEP-th row is
stored (zero and non-zero rows among them).  tests/adafactor_ref.py is held to HF's float64 result on the stored rows to float64 rounding;
the tests then take the whole-tensor float64 reference from it.  Only this script needs transformers.
"""
import json
import os

import numpy as np
import torch
from transformers.optimization import Adafactor

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1024, 64), (64, 256), (32, 8), (64,)]
STEPS = 6
ZERO_STEP = 3
SETTINGS = {
    "default": {},
    "fixed_lr": dict(lr=1e-3, relative_step=False, scale_parameter=False),
    "momentum_decay": dict(lr=1e-3, relative_step=False, beta1=0.9, weight_decay=0.01),
    "warmup": dict(warmup_init=True),
}
ROW_STEP = {0: 16, 1: 4}  # tensor index -> stored rows of p / exp_avg are [::step]
STATE_KEYS = ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq", "exp_avg")


def run(p0, grads, kw, dtype):
    ps = [torch.nn.Parameter(torch.from_numpy(a).to(dtype).clone()) for a in p0]
    opt = Adafactor(ps, **kw)
    for s in range(STEPS):
        for p, g in zip(ps, grads[s]):
            p.grad = torch.from_numpy(g).to(dtype)
        opt.step()
    return ps, opt


def main():
    rng = np.random.default_rng(20240607)
    def quant(sh, sigma):
        return np.clip(np.rint(rng.standard_normal(sh) * sigma), -127, 127).astype(np.int8)

    out, grads = {}, []
    meta = {"shapes": [list(s) for s in SHAPES], "steps": STEPS, "zero_step": ZERO_STEP, "row_step": {str(k): v for k, v in ROW_STEP.items()},
            "p0_exp": 9, "g_exp": [], "settings": {}}
    for i, sh in enumerate(SHAPES):
        out[f"p0k_{i}"] = quant(sh, 26.0)  # ~ N(0, 0.05)
    p0 = [out[f"p0k_{i}"].astype(np.float32) * np.float32(2.0 ** -meta["p0_exp"]) for i in range(len(SHAPES))]
    for s in range(STEPS):
        gs, es = [], []
        for i, sh in enumerate(SHAPES):
            k = quant(sh, 32.0)
            e = int(rng.integers(6, 16))  # |g| ~ 2**(5 - e): 0.5 ... 1e-3
            if len(sh) == 2:
                k[::3] = 0
            if s == ZERO_STEP:
                k[...] = 0
            out[f"gk_{s}_{i}"] = k
            es.append(e)
            gs.append(k.astype(np.float32) * np.float32(2.0 ** -e))
        grads.append(gs)
        meta["g_exp"].append(es)
    for name, kw in SETTINGS.items():
        ps32, o32 = run(p0, grads, kw, torch.float32)
        ps64, o64 = run(p0, grads, kw, torch.float64)
        info = {"kwargs": kw, "hf_fp32_err": [], "hf_fp32_state_err": []}
        for i, (a, b) in enumerate(zip(ps32, ps64)):
            a64, b64 = a.detach().double(), b.detach()
            assert torch.isfinite(a).all() and torch.isfinite(b).all()
            info["hf_fp32_err"].append(float((a64 - b64).norm() / (b64 - torch.from_numpy(p0[i]).double()).norm()))
            rs = ROW_STEP.get(i, 1)
            out[f"{name}_p32_{i}"] = a.detach().numpy()[::rs]
            out[f"{name}_p64_{i}"] = b.detach().numpy()[::rs]
            se = {}
            for k in STATE_KEYS:
                if k in o64.state[b]:
                    x32, x64 = o32.state[a][k], o64.state[b][k]
                    sub = slice(None, None, rs if k == "exp_avg" else 1)
                    out[f"{name}_{k}32_{i}"] = x32.numpy()[sub]
                    out[f"{name}_{k}64_{i}"] = x64.numpy()[sub]
                    se[k] = float((x32.double() - x64).norm() / x64.norm())
            out[f"{name}_rms32_{i}"] = np.float32(float(o32.state[a]["RMS"]))
            info["hf_fp32_state_err"].append(se)
        meta["settings"][name] = info
    np.savez_compressed(os.path.join(HERE, "adafactor.npz"), **out)
    with open(os.path.join(HERE, "adafactor.json"), "w") as f:
        json.dump(meta, f, indent=1)
    for name, info in meta["settings"].items():
        print(name, ["%.2e" % e for e in info["hf_fp32_err"]])


if __name__ == "__main__":
    main()
