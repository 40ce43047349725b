"""float64 restatement of the Adafactor rule (transformers.optimization.Adafactor) and the loader of tests/golden/adafactor.*
(made by tests/golden/make_adafactor_goldens.py).  No transformers, no GPU."""
import json
import math
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEFAULTS = dict(lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0.0, scale_parameter=True,
                relative_step=True, warmup_init=False)


def load_golden():
    """{shapes, steps, p0 [tensor], grads [step][tensor] (fp32, exact), settings {name: {kwargs, hf_fp32_err, ...}}, z (the npz),
    rows(i) -> the slice of tensor i's rows whose final values are stored}"""
    z = np.load(os.path.join(GOLD, "adafactor.npz"))
    meta = json.load(open(os.path.join(GOLD, "adafactor.json")))
    n = len(meta["shapes"])
    p0 = [z[f"p0k_{i}"].astype(np.float32) * np.float32(2.0 ** -meta["p0_exp"]) for i in range(n)]
    grads = [[z[f"gk_{s}_{i}"].astype(np.float32) * np.float32(2.0 ** -meta["g_exp"][s][i]) for i in range(n)] for s in range(meta["steps"])]
    for info in meta["settings"].values():
        if "eps" in info["kwargs"]:
            info["kwargs"]["eps"] = tuple(info["kwargs"]["eps"])
    return dict(shapes=[tuple(s) for s in meta["shapes"]], steps=meta["steps"], zero_step=meta["zero_step"], p0=p0, grads=grads,
                settings=meta["settings"], z=z, rows=lambda i: slice(None, None, int(meta["row_step"].get(str(i), 1))))


def new_state(p, beta1):
    st = {"step": 0, "RMS": 0.0}
    if p.ndim >= 2:
        st["exp_avg_sq_row"] = np.zeros(p.shape[:-1])
        st["exp_avg_sq_col"] = np.zeros(p.shape[:-2] + p.shape[-1:])
    else:
        st["exp_avg_sq"] = np.zeros(p.shape)
    if beta1 is not None:
        st["exp_avg"] = np.zeros(p.shape)
    return st


def step_tensor(p, g, st, **kw):
    """one Adafactor step of one tensor in float64: returns the new p, updates st in place"""
    o = dict(DEFAULTS, **kw)
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    eps0, eps1 = o["eps"]
    st["step"] = t = st["step"] + 1
    st["RMS"] = rms_p = math.sqrt(float((p * p).sum()) / p.size)
    rel = min(1e-6 * t if o["warmup_init"] else 1e-2, 1.0 / math.sqrt(t)) if o["relative_step"] else o["lr"]
    lr_t = rel * (max(eps1, rms_p) if o["scale_parameter"] else 1.0)
    beta2t = 1.0 - t ** o["decay_rate"]
    sq = g * g + eps0
    if p.ndim >= 2:
        st["exp_avg_sq_row"] = R = beta2t * st["exp_avg_sq_row"] + (1.0 - beta2t) * sq.mean(-1)
        st["exp_avg_sq_col"] = C = beta2t * st["exp_avg_sq_col"] + (1.0 - beta2t) * sq.mean(-2)
        u = g / np.sqrt(R / R.mean(-1, keepdims=True))[..., None] / np.sqrt(C)[..., None, :]
    else:
        st["exp_avg_sq"] = V = beta2t * st["exp_avg_sq"] + (1.0 - beta2t) * sq
        u = g / np.sqrt(V)
    rms_u = math.sqrt(float((u * u).sum()) / u.size)
    u = u / max(1.0, rms_u / o["clip_threshold"]) * lr_t
    if o["beta1"] is not None:
        st["exp_avg"] = u = o["beta1"] * st["exp_avg"] + (1.0 - o["beta1"]) * u
    if o["weight_decay"] != 0:
        p = p - o["weight_decay"] * lr_t * p
    return p - u


def run_f64(p0, grads, **kw):
    """all steps of all tensors: (final params, states)"""
    ps = [np.asarray(p, np.float64) for p in p0]
    sts = [new_state(p, dict(DEFAULTS, **kw)["beta1"]) for p in ps]
    for gs in grads:
        ps = [step_tensor(p, g, st, **kw) for p, g, st in zip(ps, gs, sts)]
    return ps, sts


def displacement_err(x, ref64, p0):
    """||x - ref|| / ||ref - p0||: the error in units of how far the optimizer moved the tensor"""
    x, ref64, p0 = (np.asarray(a, np.float64) for a in (x, ref64, p0))
    return float(np.linalg.norm(x - ref64) / np.linalg.norm(ref64 - p0))


def rel_err(x, ref64):
    x, ref64 = np.asarray(x, np.float64), np.asarray(ref64, np.float64)
    return float(np.linalg.norm(x - ref64) / np.linalg.norm(ref64))
