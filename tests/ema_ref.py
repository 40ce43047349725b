"""The fp64 reference and the per-element bound for the fused weight EMA (csrc/ema.hip, optim.WeightEMA), shared by
tests/test_ema_cpu.py (which shows that three f32 evaluations of the rule stay inside the bound) and tests/test_ema_gpu.py (which
holds the kernel and the class to it).  Plain torch / numpy on the CPU.

With w the f32 scalar the kernel receives and ref = e + w (p - e) in fp64:

    |got - ref| <= 1.01 * 2^-24 * (2 w |p - e| + |ref|) + 2^-149

One rounding of p - e, scaled by w; one of the product w * (p - e); one of the sum.  A fused multiply-add drops the middle term.
The factor 1.01 covers the second-order terms, 2^-149 a result in the denormal range."""
import numpy as np
import torch

from tests.engine_kernels_ref import U24

f32 = lambda a: float(np.float32(a))

W_POW2 = 2.0 ** -10
W_999 = f32(1.0 - 0.999)
WEIGHTS = (W_POW2, W_999)  # what the GPU kernel tests run with


def decay_at(decay, warmup, t):
    """decay_t of update number t (1-based), in double"""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def weight_at(decay, warmup, t):
    """w of update number t: float32(1.0 - decay_t), formed in double"""
    return f32(1.0 - decay_at(decay, warmup, t))


def ema_ref(p, e, w):
    """(ref, bound): the fp64 update of shadow e towards p with the f32 scalar w, and the per-element bound above"""
    p, e = p.double(), e.double()
    ref = e + w * (p - e)
    return ref, 1.01 * U24 * (2.0 * w * (p - e).abs() + ref.abs()) + 2.0 ** -149


def worst(got, p, e, w):
    """the worst error of `got` as a fraction of its bound"""
    ref, bound = ema_ref(p, e, w)
    return float(((got.double() - ref).abs() / bound).max())


def must_move(p, e, w):
    """elements whose f32 result cannot equal e: ref is further from e than the bound and one spacing of f32 at e together.
    (w |p - e| below half a spacing of e rounds back to e in any correct f32 evaluation: 'moved' can be asked only of these.)"""
    ref, bound = ema_ref(p, e, w)
    return (ref - e.double()).abs() > bound + 2.0 * U24 * e.double().abs() + 2.0 ** -149


# ---- three f32 evaluations of the rule -----------------------------------------------------------------------------------------------
def ema_plain(p, e, w):
    """every operation rounded to f32, no fused multiply-add"""
    w = torch.tensor(w, dtype=torch.float32)
    return e + w * (p - e)


def ema_fma(p, e, w):
    """the difference rounded to f32, then one fused multiply-add: the product of two f32 is exact in fp64, its sum with e is
    rounded to fp64 and then to f32 (the double rounding moves a result by far less than the bound's 1 %)"""
    d = (p - e).double()
    return (e.double() + w * d).float()


def ema_lerp(p, e, w):
    return torch.lerp(e, p, w)


FORMS = {"plain": ema_plain, "fma": ema_fma, "lerp": ema_lerp}


def recurrence(params_per_update, e0, decay, warmup):
    """the fp64 recurrence over a list of parameter tensors (one per update) and the accumulated bound of an f32 evaluation that meets
    the single-step bound at every update: acc_t = (1 - w_t) acc_{t-1} + b_t, with b_t the single-step bound evaluated at the worst
    inputs the f32 shadow may hold (|p - e| and |ref| each enlarged by acc_{t-1})"""
    e = e0.double()
    acc = torch.zeros_like(e)
    for t, p in enumerate(params_per_update, start=1):
        w = weight_at(decay, warmup, t)
        ref = e + w * (p.double() - e)
        b = 1.01 * U24 * (2.0 * w * ((p.double() - e).abs() + acc) + ref.abs() + acc) + 2.0 ** -149
        acc = (1.0 - w) * acc + b
        e = ref
    return e, acc
