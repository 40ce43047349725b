"""Gradient-norm clipping without a GPU: the numpy reference of tests/grad_clip_ref.py against torch.nn.utils.clip_grad_norm_,
optim.clip_grad_norm_'s delegation to torch wherever the kernels do not apply, and the host side of the gradient table."""
import math

import numpy as np
import pytest
import torch

from tests import grad_clip_ref as R

SHAPES = [(1,), (3,), (17, 5), (1021,), (64, 33), (9000,)]  # <= 1e4 elements each: n * 2^-53 is far below the 1e-12 asked for


def _grads(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(s) * scale).astype(np.float32) for s in SHAPES]


def _params(grads, dtype=torch.float32):
    ps = []
    for g in grads:
        p = torch.nn.Parameter(torch.zeros(g.shape, dtype=dtype))
        p.grad = torch.from_numpy(np.array(g)).to(dtype)
        ps.append(p)
    return ps


@pytest.mark.parametrize("norm_type", [2.0, math.inf])
@pytest.mark.parametrize("clipped", [True, False])
def test_reference_agrees_with_torch_in_float64(norm_type, clipped):
    grads = _grads(1)
    per, total = R.norms(grads, norm_type)
    max_norm = total * (0.37 if clipped else 3.0)
    ps = _params(grads, torch.float64)
    want_per = [float(torch.linalg.vector_norm(p.grad, norm_type)) for p in ps]
    got = torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type)
    assert abs(float(got) - total) <= 1e-12 * total
    for a, b in zip(per, want_per):
        assert abs(a - b) <= 1e-12 * b
    c64 = min(max_norm / (total + 1e-6), 1.0)
    assert (c64 < 1.0) == clipped
    for p, g in zip(ps, grads):
        want = g.astype(np.float64) * c64
        assert np.allclose(p.grad.numpy(), want, rtol=1e-12, atol=0.0)
    # the fp32 coefficient is the float64 one up to fp32 rounding: the total's, the sum's, the quotient's (1.5 ulp = 1.8e-7)
    c32 = float(R.coef(total, max_norm))
    assert abs(c32 - c64) <= 2e-7 * c64


@pytest.mark.parametrize("norm_type", [2.0, math.inf])
@pytest.mark.parametrize("bad,where", [(float("nan"), 0), (float("nan"), -1), (float("inf"), 0), (float("-inf"), 4321)])
def test_reference_nonfinite_equals_torch_fp32(norm_type, bad, where):
    grads = _grads(2)
    grads[5][where] = bad
    total, c, want = R.clip(grads, 1.0, norm_type)
    ps = _params(grads)
    got = torch.nn.utils.clip_grad_norm_(ps, 1.0, norm_type)
    if math.isnan(bad):
        assert math.isnan(total) and math.isnan(float(got)) and math.isnan(float(c))
        for p in ps:
            assert torch.isnan(p.grad).all()  # NaN coefficient: every gradient of every tensor
    else:
        assert total == math.inf and float(got) == math.inf and float(c) == 0.0
        for p, w in zip(ps, want):
            assert np.array_equal(p.grad.numpy(), w, equal_nan=True)
        assert math.isnan(float(ps[5].grad.reshape(-1)[where]))  # inf * 0
        assert float(ps[0].grad.abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="is non-finite, so it cannot be clipped"):
        torch.nn.utils.clip_grad_norm_(_params(grads), 1.0, norm_type, error_if_nonfinite=True)


def _same_as_torch(make, *args, **kw):
    from klab_multimodalmodel_amd import optim
    a, b = make(), make()
    ra = optim.clip_grad_norm_(a, *args, **kw)
    rb = torch.nn.utils.clip_grad_norm_(b, *args, **kw)
    assert ra.dtype == rb.dtype and ra.shape == rb.shape and ra.device == rb.device
    assert torch.equal(ra, rb) or (torch.isnan(ra).all() and torch.isnan(rb).all())
    for p, q in zip(a, b):
        if q.grad is None:
            assert p.grad is None
        else:
            assert p.grad.dtype == q.grad.dtype and torch.equal(p.grad, q.grad)
    return ra


@pytest.mark.parametrize("norm_type", [2.0, math.inf, 1.0, 3.5])
@pytest.mark.parametrize("max_norm", [0.5, 1e9])
def test_cpu_parameters_delegate_bit_identically(norm_type, max_norm):
    _same_as_torch(lambda: _params(_grads(3)), max_norm, norm_type)
    _same_as_torch(lambda: _params(_grads(3)), max_norm, norm_type=norm_type, foreach=False)


def test_mixed_float64_gradient_delegates_bit_identically():
    def make():
        grads = _grads(4)
        ps = _params(grads)
        ps[2] = _params([grads[2]], torch.float64)[0]
        return ps
    _same_as_torch(make, 0.25)
    _same_as_torch(make, 0.25, math.inf)


def test_none_gradients_empty_list_and_single_tensor():
    from klab_multimodalmodel_amd import optim

    def make():
        ps = _params(_grads(5))
        ps[1].grad = None
        ps[4].grad = None
        return ps
    _same_as_torch(make, 0.1)
    for empty in ([], [torch.nn.Parameter(torch.zeros(3))]):  # nothing at all / no gradient at all
        r = optim.clip_grad_norm_(empty, 1.0)
        w = torch.nn.utils.clip_grad_norm_(empty, 1.0)
        assert torch.equal(r, w) and r.dtype == w.dtype and r.device == w.device and float(r) == 0.0
    # a single tensor and a generator are accepted as in torch
    a, b = _params(_grads(6))[3], _params(_grads(6))[3]
    assert torch.equal(optim.clip_grad_norm_(a, 0.5), torch.nn.utils.clip_grad_norm_(b, 0.5)) and torch.equal(a.grad, b.grad)
    c, d = _params(_grads(6)), _params(_grads(6))
    assert torch.equal(optim.clip_grad_norm_((p for p in c), 0.5), torch.nn.utils.clip_grad_norm_((p for p in d), 0.5))
    for p, q in zip(c, d):
        assert torch.equal(p.grad, q.grad)


def test_error_if_nonfinite_on_delegation_path():
    from klab_multimodalmodel_amd import optim
    grads = _grads(7)
    grads[0][0] = float("nan")
    with pytest.raises(RuntimeError, match="is non-finite, so it cannot be clipped"):
        optim.clip_grad_norm_(_params(grads), 1.0, error_if_nonfinite=True)


def test_grad_norms_needs_the_native_path():
    from klab_multimodalmodel_amd import optim
    with pytest.raises(NotImplementedError):
        optim.grad_norms(_params(_grads(8)))


def test_table_plan_counts_and_owners():
    """tensor i owns ceil(n_i / chunk) consecutive partials, in table order, for every length at which the kernels change path"""
    from klab_multimodalmodel_amd.build import build_library
    build_library(verbose=False)
    from klab_multimodalmodel_amd import ops
    c = ops.grad_norm_chunk()
    assert c >= 1024 and c % 4 == 0  # whole 16-byte vectors: a chunk keeps its tensor's alignment
    numels = [1, 3, 4, 5, 1021, c - 1, c, c + 1, 2 * c + 3]
    want_counts = [1, 1, 1, 1, 1, 1, 1, 2, 3]
    first, nparts = ops.grad_norm_plan(numels)
    assert nparts == sum(want_counts) == 12
    assert first == [0, 1, 2, 3, 4, 5, 6, 7, 9]
    owners = [i for i, k in enumerate(want_counts) for _ in range(k)]
    for part in range(nparts):  # the owner of a partial is the last tensor whose first partial is not after it (the kernels' search)
        assert max(i for i, f in enumerate(first) if f <= part) == owners[part]
    assert ops.grad_norm_plan(numels, chunk=4) == ([0, 1, 2, 3, 5, 261, 261 + (c - 1 + 3) // 4, 261 + (c - 1 + 3) // 4 + c // 4,
                                                    261 + (c - 1 + 3) // 4 + c // 4 + (c + 4) // 4],
                                                   261 + (c - 1 + 3) // 4 + c // 4 + (c + 4) // 4 + (2 * c + 6) // 4)
    assert ops.grad_norm_plan([]) == ([], 0)
    assert ops.grad_norm_plan([9] * 1025, chunk=c) == (list(range(1025)), 1025)
    with pytest.raises(ValueError):
        ops.grad_norm_plan([5, 0, 7])
