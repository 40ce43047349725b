#!/usr/bin/env python3
"""klab_t5_attn_bwd_fused against the two launches it replaces (o / co dgrad GEMM + t5_attn_bwd; T5-small, B = 64): device time per
call from HIP events."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from klab_multimodalmodel_amd import ops  # noqa: E402


def timeit(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def main():
    dt = torch.bfloat16
    B, H, dk, d = 64, 8, 64, 512
    inner = H * dk
    for name, Lq, Lk, cross, causal in (("dec self", 64, 64, False, True), ("enc self", 58, 58, False, False), ("dec cross", 64, 58, True, False)):
        w = (torch.randn(d, inner, device="cuda") * d ** -0.5).to(dt)
        dy = torch.randn(B * Lq, d, device="cuda").to(dt)
        if cross:
            qb = (torch.randn(B * Lq, inner, device="cuda") * 0.5).to(dt)
            kvb = (torch.randn(B * Lk, 2 * inner, device="cuda") * 0.5).to(dt)
            q, k, v, ldq, ldkv = qb, kvb[:, :inner], kvb[:, inner:], inner, 2 * inner
            dqb = torch.empty(B * Lq, inner, device="cuda", dtype=dt)
            dkvb = torch.empty(B * Lk, 2 * inner, device="cuda", dtype=dt)
            dq, dkk, dv = dqb, dkvb[:, :inner], dkvb[:, inner:]
        else:
            qb = (torch.randn(B * Lq, 3 * inner, device="cuda") * 0.5).to(dt)
            q, k, v, ldq, ldkv = qb, qb[:, inner:], qb[:, 2 * inner:], 3 * inner, 3 * inner
            dqkv = torch.empty(B * Lq, 3 * inner, device="cuda", dtype=dt)
            dq, dkk, dv = dqkv, dqkv[:, inner:], dqkv[:, 2 * inner:]
        bias = None if cross else torch.randn(H, Lq, Lk, device="cuda")
        dbias = None if cross else torch.zeros(H, Lq, Lk, device="cuda")
        ds_ws = None if cross else torch.empty(B * H * Lq * ((Lk + 31) // 32 * 32), device="cuda", dtype=dt)
        sd = torch.tensor([5], dtype=torch.int32, device="cuda")
        kw = dict(B=B, H=H, Lq=Lq, Lk=Lk, dk=dk, bias=bias, causal=causal, drop_p=0.1, seed=sd, tag=3)
        ctx = torch.empty(B * Lq, inner, device="cuda", dtype=dt)
        lse = torch.empty(B, H, Lq, device="cuda")
        ops.t5_attn_fwd(q, k, v, ctx, lse, ldq=ldq, ldk=ldkv, ldv=ldkv, **kw)
        dctx = torch.empty(B * Lq, inner, device="cuda", dtype=dt)
        ld = dict(ldq=ldq, ldk=ldkv, ldv=ldkv, lddq=dq.stride(0), lddk=dkk.stride(0), lddv=dv.stride(0))

        # (ds_ws with the reduction deferred, as the engine runs the self-attention backward)
        def two():
            ops.gemm(dy, w, dctx, M=B * Lq, N=inner, K=d, a_kmajor=True, b_kmajor=False, ldb=inner)
            a = ops._attn_args(q, k, v, ctx, lse, bias, causal, B, H, Lq, Lk, dk, 0.1, sd, 3, ldq, ldkv, ldkv, inner)
            a.dctx, a.lddo = dctx.data_ptr(), inner
            a.dq, a.lddq, a.dk_out, a.lddk, a.dv, a.lddv = dq.data_ptr(), ld["lddq"], dkk.data_ptr(), ld["lddk"], dv.data_ptr(), ld["lddv"]
            a.dbias, a.ds_ws, a.ds_defer = ops.L.ptr(dbias), ops.L.ptr(ds_ws), 1
            ops.L.check(ops.L.load().klab_t5_attn_bwd(ops.C.byref(a), ops.L.stream_ptr()), "klab_t5_attn_bwd")

        def fused():
            ops.t5_attn_bwd_fused(dy, w, q, k, v, ctx, lse, dq, dkk, dv, dbias=dbias, ds_ws=ds_ws, ds_defer=True, **ld, **kw)

        res = {"two": [], "fused": []}
        for _ in range(3):
            res["two"].append(timeit(two))
            res["fused"].append(timeit(fused))
        t2, tf = sorted(res["two"])[1], sorted(res["fused"])[1]
        print(f"{name:10s} dgrad + attn bwd {t2:7.1f} us   fused {tf:7.1f} us   ratio {tf / t2:.2f}", flush=True)


if __name__ == "__main__":
    main()
