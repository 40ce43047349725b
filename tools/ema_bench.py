#!/usr/bin/env python3
"""Time of the fused weight EMA on one MI355X, on the optimizer table of a real binding (Swin-V2 C=64 frozen + a T5), in one process:

  (a) adamw     klab_engine_adamw_step with the two groups of optim.decay_param_groups: the yardstick, 30 bytes per parameter
  (b) update    klab_engine_ema_update: p, e in, e out -- 12 bytes per parameter
  (c) swap      klab_engine_ema_swap: p, e in, p, e out and the bf16 copy of the GEMM weights -- 16 + 2 bytes per parameter
  (d) foreach   torch._foreach_lerp_(shadows, params, w) over the same tensors: the same 12 bytes, one launch per chunk of tensors

--t5 small is the BASELINE configs[1] workload of bench.py (B = 64); --t5 base / large take the towers of bench.py's cfg3 / cfg5
workloads (Swin frozen, random weights) and bind them at B = 2: only the table and the parameter bytes matter to what is timed
here.

The forms are interleaved in rounds and the form a round begins with rotates.  Before every timed call, outside the timed span, an
8192^2 fp32 product runs: it pushes the buffers out of the caches and keeps the device busy for ~10 ms, so the host has finished
enqueueing the call before the device reaches the first event -- the events then bracket device time alone.  The host column is
the time the call itself takes to return (enqueue cost), measured in the same rounds.

    python tools/ema_bench.py [--t5 small|base|large] [--out profiles/ema.txt]
"""
import argparse
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOAD_OF = {"small": "caption", "base": "cfg3", "large": "cfg5"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--t5", default="small", choices=["small", "base", "large"])
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--out", default=None, help="also append the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench needs the GPU: nothing is measured without one")
    import bench
    from klab_multimodalmodel_amd import optim
    from klab_multimodalmodel_amd.models.model import MyModel
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    w = bench.WORKLOADS[WORKLOAD_OF[a.t5]]
    sw, t5 = bench.workload_configs(WORKLOAD_OF[a.t5])
    B = w["B"] if a.t5 == "small" else 2
    m = MyModel(args, _configs=(sw, t5, t5), _seed=0, dtype="bf16").to("cuda")
    m._direct_grads = True
    m.transformer.train()
    pix, src, tgt = bench.synth_batch(B, w["Ls"], w["Lt"], sw.image_size, m.main_cfg.vocab_size, "cuda")
    m({"pixel_values": pix}, {"input_ids": src}, {"input_ids": tgt}).backward()
    eng, flat = m._engine, m.flat_grads("main")
    groups = optim.decay_param_groups(m, 0.01)
    params = [p for g in groups for p in g["params"]]
    n_el = sum(p.numel() for p in params)
    n_copy = sum(p.numel() for p in params if p.dim() >= 2)
    ptrs, _n0 = eng.adam_layout()
    by_ptr = {p.data_ptr(): k for k, g in enumerate(groups) for p in g["params"]}
    gid2 = torch.tensor([by_ptr[q] for q in ptrs], dtype=torch.int32, device="cuda")
    mom, var = torch.zeros_like(flat), torch.zeros_like(flat)
    hyper = lambda wd, t: dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd, bias_corr1=1 - 0.9 ** t, bias_corr2=1 - 0.999 ** t)
    ema = torch.zeros_like(flat)
    datas = [p.data for p in params]
    shadows = [p.detach().clone() for p in params]
    wt = 1.0 - 0.999

    step = [1]
    calls = {
        "a adamw, 2 groups": lambda: eng.adamw_step(mom, var, gid2, [hyper(0.01, step[0]), hyper(0.0, step[0])]),
        "b ema update": lambda: eng.ema_update(ema, wt),
        "c ema swap": lambda: eng.ema_swap(ema),
        "d torch._foreach_lerp_": lambda: torch._foreach_lerp_(shadows, datas, wt),
    }
    nbytes = {"a": 30 * n_el, "b": 12 * n_el, "c": 16 * n_el + 2 * n_copy, "d": 12 * n_el}
    busy = torch.randn(8192, 8192, device="cuda")
    dev, host = {k: [] for k in calls}, {k: [] for k in calls}
    for r in range(a.warm + a.n):
        step[0] = r + 1
        order = list(calls.items())
        order = order[r % len(order):] + order[:r % len(order)]  # every form takes every place in the round equally often
        for k, fn in order:
            torch.mm(busy, busy)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warm:
                dev[k].append(e0.elapsed_time(e1) * 1e3)
                host[k].append((t1 - t0) * 1e6)
    finite = all(bool(torch.isfinite(p).all()) for p in params) and bool(torch.isfinite(ema).all())
    lines = [f"Weight EMA, t5-{a.t5} (B={B}): {len(ptrs)} tensors, N = {n_el} elements ({n_copy} with a bf16 copy)",
             f"median (min) of {a.n} interleaved rounds (rotating order) after {a.warm} warm-up; device us between events behind a 10 ms product, "
             f"caches flushed; host us = the call's own return time",
             f"{'':24s} {'device us':>18s} {'host us':>9s} {'bytes':>10s} {'GB/s':>8s}"]
    for k in calls:
        nb = nbytes[k[0]]
        d, dm = statistics.median(dev[k]), min(dev[k])
        lines.append(f"{k:24s} {d:9.1f} ({dm:7.1f}) {statistics.median(host[k]):9.1f} {nb / 1e6:8.1f}MB {nb / d / 1e3:8.0f}")
    blocks = [statistics.median(dev["a adamw, 2 groups"][i:i + 10]) for i in range(0, a.n - 9, 10)]
    da, db, dc, dd = (statistics.median(dev[k]) for k in calls)
    lines.append(f"(a)'s medians over blocks of 10 rounds: {', '.join(f'{b:.1f}' for b in blocks)}: spread {max(blocks) - min(blocks):.1f} us")
    lines.append(f"(b) / (a) = {db / da:.3f} (by bytes 12 / 30 = 0.400)   (c) / (a) = {dc / da:.3f} (by bytes {nbytes['c'] / nbytes['a']:.3f})   "
                 f"(d) / (b) = {dd / db:.2f}   (device medians)")
    lines.append(f"check: parameters and shadow finite after {a.warm + a.n} rounds (an odd number of swaps leaves them exchanged): {finite}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
