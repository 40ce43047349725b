#!/usr/bin/env python3
"""Time of the fused AdamW step on one MI355X at the BASELINE configs[1] sizes (Swin-V2 C=64 frozen + t5-small, B=64), on the
gradients of one real forward + backward, in one process:

  (a) adam      klab_engine_adam_step: the existing one-group Adam kernel, the yardstick
  (b) adamw 1   klab_engine_adamw_step with one parameter group
  (c) adamw 2   klab_engine_adamw_step with the two groups of optim.decay_param_groups
  (d) torch     torch.optim.AdamW(fused=True) on the same two groups, followed by the fp32 -> bf16 cast of the GEMM weights
                that the next forward then needs (klab_cast_pack into one buffer)

The four are interleaved in rounds, and the form a round begins with rotates: in a fixed order (a) always ran behind (d) and
measured 3.4 us (1.2 %) above (b) and (c), a difference that went away with the rotation.  Before every timed call, outside the
timed span, an 8192^2 fp32 product runs: it pushes the buffers out of the caches and keeps the device busy for ~10 ms, so the
host has finished enqueueing the call before the device reaches the first event -- the events then bracket device time alone.

Bytes: (a) - (c) read p, g, m, v and write p, m, v and the bf16 copy: 30 per parameter.  (d): 28, and 6 more for the cast.
The spread of (a) is the range of its medians over consecutive blocks of ten rounds: what two runs of the SAME kernel differ by.

    python tools/adamw_bench.py [--out profiles/adamw.txt]
"""
import argparse
import os
import statistics
import sys
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
        raise SystemExit("adamw_bench needs the GPU: nothing is measured without one")
    import bench
    from klab_multimodalmodel_amd import ops, optim
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
    eng, flat = m._engine, m.flat_grads("main")
    groups = optim.decay_param_groups(m, 0.01)
    params = [p for g in groups for p in g["params"]]
    n_el = sum(p.numel() for p in params)
    ptrs, n0 = eng.adam_layout()
    by_ptr = {p.data_ptr(): k for k, g in enumerate(groups) for p in g["params"]}
    gid2 = torch.tensor([by_ptr[q] for q in ptrs], dtype=torch.int32, device="cuda")
    gid1 = torch.zeros_like(gid2)
    mom, var = torch.zeros_like(flat), torch.zeros_like(flat)
    hyper = lambda wd, t: dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd, bias_corr1=1 - 0.9 ** t, bias_corr2=1 - 0.999 ** t)
    topt = torch.optim.AdamW(groups, lr=1e-4, fused=True)
    mats = [p for p in params if p.dim() >= 2]
    pre, rows = 0, []
    for p in mats:
        rows.append([p.data_ptr(), 4 * pre, pre])
        pre += p.numel() // 4
    cast_desc = torch.tensor(rows, dtype=torch.int64, device="cuda")
    cast_dst = torch.empty(4 * pre, dtype=torch.bfloat16, device="cuda")

    def torch_step():
        topt.step()
        ops.cast_pack(cast_desc, pre, cast_dst)

    step = [1]
    calls = {
        "a adam (yardstick)": lambda: eng.adam_step(mom, var, 1e-4, 0.9, 0.999, 1e-8, 0.0, 1 - 0.9 ** step[0], 1 - 0.999 ** step[0]),
        "b adamw, 1 group": lambda: eng.adamw_step(mom, var, gid1, [hyper(0.01, step[0])]),
        "c adamw, 2 groups": lambda: eng.adamw_step(mom, var, gid2, [hyper(0.01, step[0]), hyper(0.0, step[0])]),
        "d torch fused + cast": torch_step,
    }
    busy = torch.randn(8192, 8192, device="cuda")
    dev = {k: [] for k in calls}
    for r in range(a.warm + a.n):
        step[0] = r + 1
        order = list(calls.items())
        order = order[r % len(order):] + order[:r % len(order)]  # every form takes every place in the round equally often
        for k, fn in order:
            torch.mm(busy, busy)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warm:
                dev[k].append(e0.elapsed_time(e1) * 1e3)
    finite = all(bool(torch.isfinite(p).all()) for p in params)
    lines = [f"AdamW step, BASELINE configs[1] (t5-small, B={w['B']}): {len(ptrs)} tensors ({n0} in backward segment 0), N = {n_el} elements, "
             f"groups of {len(groups[0]['params'])} + {len(groups[1]['params'])} tensors",
             f"median (min) of {a.n} interleaved rounds (rotating order) after {a.warm} warm-up; device us between events behind a 10 ms product, caches flushed",
             f"{'':24s} {'device us':>18s} {'bytes':>10s} {'GB/s':>8s}"]
    for k in calls:
        nb = (34 if k.startswith("d") else 30) * n_el
        d, dm = statistics.median(dev[k]), min(dev[k])
        lines.append(f"{k:24s} {d:9.1f} ({dm:7.1f}) {nb / 1e6:8.1f}MB {nb / d / 1e3:8.0f}")
    blocks = [statistics.median(dev["a adam (yardstick)"][i:i + 10]) for i in range(0, a.n - 9, 10)]
    da, db, dc, dd = (statistics.median(dev[k]) for k in calls)
    lines.append(f"(a)'s medians over blocks of 10 rounds: {', '.join(f'{b:.1f}' for b in blocks)}: spread {max(blocks) - min(blocks):.1f} us")
    lines.append(f"(b) - (a) = {db - da:+.1f} us   (c) - (a) = {dc - da:+.1f} us   (d) / (c) = {dd / dc:.2f}   (device medians)")
    lines.append(f"check: every parameter finite after {4 * (a.warm + a.n)} updates: {finite}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
