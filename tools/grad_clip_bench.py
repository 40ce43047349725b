#!/usr/bin/env python3
"""Time of gradient-norm clipping on one MI355X at the BASELINE configs[1] sizes (Swin-V2 C=64 frozen + t5-small, B=64), on the
gradients of one real forward + backward, in one process:

  (a) torch     torch.nn.utils.clip_grad_norm_ over the .grad views (its scale pass always runs)
  (b) native    optim.clip_grad_norm_ with a max_norm the gradients stay under: the norm, and a scale launch that stores nothing
  (c) native    optim.clip_grad_norm_ with max_norm = half the norm: the norm and the scale

The three are interleaved in rounds.  Before every timed call, outside the timed span, the gradients are restored from a copy
(so (c) clips the same values every time) and an 8192^2 fp32 product runs: it pushes the gradients out of the caches, and it
keeps the device busy for ~10 ms, so the host has finished enqueueing the call before the device reaches the first event --
the events then bracket device time alone.  The wall figure has a device synchronisation on both sides and no product in
front: it includes the host's work (torch's path launches per group of tensors; ours walks the parameter list once).

Bytes: N gradient elements; the norm reads 4 N, the scale reads and writes 8 N more.

    python tools/grad_clip_bench.py [--out profiles/grad_clip.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grad_clip_bench needs the GPU: nothing is measured without one")
    import bench
    from klab_multimodalmodel_amd import optim
    from klab_multimodalmodel_amd.models.model import MyModel
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    w = bench.WORKLOADS["caption"]
    sw, t5 = bench.workload_configs("caption")
    m = MyModel(args, _configs=(sw, t5, t5), _seed=0, dtype="bf16").to("cuda")
    m._direct_grads = True
    m.transformer.train()
    pix, src, tgt = bench.synth_batch(w["B"], w["Ls"], w["Lt"], sw.image_size, m.main_cfg.vocab_size, "cuda")
    m({"pixel_values": pix}, {"input_ids": src}, {"input_ids": tgt}).backward()
    params = [p for p in m.transformer.parameters() if p.grad is not None]
    flat = m.flat_grads("main")
    keep = flat.clone()
    n_el = sum(p.grad.numel() for p in params)
    norm = float(optim.clip_grad_norm_(params, 1e30))
    busy = torch.randn(8192, 8192, device="cuda")
    calls = {
        "a torch, not clipped": lambda: torch.nn.utils.clip_grad_norm_(params, 1e30),
        "b native, not clipped": lambda: optim.clip_grad_norm_(params, 1e30),
        "c native, clipped": lambda: optim.clip_grad_norm_(params, 0.5 * norm),
        "a' torch, clipped": lambda: torch.nn.utils.clip_grad_norm_(params, 0.5 * norm),
    }
    dev = {k: [] for k in calls}
    wall = {k: [] for k in calls}
    for r in range(a.warm + a.n):
        for k, fn in calls.items():
            flat.copy_(keep)
            torch.mm(busy, busy)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warm:
                dev[k].append(e0.elapsed_time(e1) * 1e3)
            flat.copy_(keep)
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= a.warm:
                wall[k].append((time.perf_counter() - t) * 1e6)
    # the clipped call really clipped, the other one changed nothing
    flat.copy_(keep)
    calls["b native, not clipped"]()
    same = bool(torch.equal(flat, keep))
    calls["c native, clipped"]()
    ratio = float(flat.double().norm() / keep.double().norm())
    lines = [f"gradient clipping, BASELINE configs[1] (t5-small, B={w['B']}): {len(params)} gradient tensors, N = {n_el} elements "
             f"({4 * n_el / 1e6:.1f} MB), total norm {norm:.4g}",
             f"median (min) of {a.n} interleaved rounds after {a.warm} warm-up; device us between events behind a 10 ms product, "
             "caches flushed; wall us with a synchronise on both sides",
             f"{'':24s} {'device us':>18s} {'bytes':>10s} {'GB/s':>8s} {'wall us':>18s}"]
    for k in calls:
        nb = (4 if "not clipped" in k and "native" in k else 12) * n_el
        d, dm = statistics.median(dev[k]), min(dev[k])
        wl, wm = statistics.median(wall[k]), min(wall[k])
        lines.append(f"{k:24s} {d:9.1f} ({dm:7.1f}) {nb / 1e6:8.1f}MB {nb / d / 1e3:8.0f} {wl:9.1f} ({wm:7.1f})")
    da, db, dc = (statistics.median(dev[k]) for k in list(calls)[:3])
    lines.append(f"(b) / (a) = {db / da:.2f}   (c) / (a) = {dc / da:.2f}   (device medians)")
    lines.append(f"check: (b) left every gradient bit unchanged: {same}; after (c) |g| / |g0| = {ratio:.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
