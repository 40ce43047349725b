#!/usr/bin/env python3
"""Time of the two LoRA kernels on one MI355X, on the adapter table of a real binding (Swin-V2 frozen + a T5), in one process, for
targets ("q", "v") and "all-linear" at r = 8 and 64:

  (a) merge        klab_lora_merge over the table into a bf16 arena: 4 B in and 2 B out per element of the targets
  (b) grads        klab_lora_grads, both launches: dW read once (4 B per element), the dA partials written and read back
  (c) torch merge  per tensor torch.addmm(W, B, A, alpha=s) into a temporary plus the cast into the arena slice
  (d) torch grads  per tensor two torch.mm (B^T dW and dW A^T) times s

and, with --step, the whole training step of the bound workload: full fine-tuning with optim.FusedAdam (for context) against
adapters with torch.optim.AdamW.

--t5 small is the BASELINE configs[1] workload of bench.py (B = 64); --t5 large takes the towers of bench.py's cfg5 workload and binds
them at B = 2: only the table and the parameter bytes matter to the kernel times.  The forms are interleaved in rounds with a
rotating start; before every timed call an 8192^2 fp32 product pushes the buffers out of the caches and keeps the device busy for
~10 ms, so the events bracket device time alone (tools/ema_bench.py).  The byte floor is the bytes each form must move at the
6.29 TB/s a float4 copy measures on this chip.

    python tools/lora_bench.py [--t5 small|large] [--step] [--out profiles/lora.txt]
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

WORKLOAD_OF = {"small": "caption", "large": "cfg5"}
COPY_RATE = 6.29e12


def timed(calls, warm, n):
    busy = torch.randn(8192, 8192, device="cuda")
    dev = {k: [] for k in calls}
    for r in range(warm + n):
        order = list(calls.items())
        order = order[r % len(order):] + order[:r % len(order)]
        for k, fn in order:
            torch.mm(busy, busy)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warm:
                dev[k].append(e0.elapsed_time(e1) * 1e3)
    return dev


def step_time(m, batch, opt, steps, warm):
    pix, src, tgt = batch
    for i in range(warm + steps):
        if i == warm:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        m({"pixel_values": pix}, {"input_ids": src}, {"input_ids": tgt}).backward()
        opt.step()
        opt.zero_grad()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--t5", default="small", choices=["small", "large"])
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="also time the whole training step")
    ap.add_argument("--out", default=None, help="also append the tables to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_bench needs the GPU: nothing is measured without one")
    import bench
    from klab_multimodalmodel_amd import lora, ops, optim
    from klab_multimodalmodel_amd.models.model import MyModel
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    w = bench.WORKLOADS[WORKLOAD_OF[a.t5]]
    sw, t5 = bench.workload_configs(WORKLOAD_OF[a.t5])
    B = w["B"] if a.t5 == "small" else 2
    m = MyModel(args, _configs=(sw, t5, t5), _seed=0, dtype="bf16").to("cuda")
    m._direct_grads = True
    m.transformer.train()
    batch = bench.synth_batch(B, w["Ls"], w["Lt"], sw.image_size, m.main_cfg.vocab_size, "cuda")
    pix, src, tgt = batch
    lines = []
    if a.step:
        opt = optim.FusedAdam(m.transformer.parameters(), lr=1e-4)
        full = step_time(m, batch, opt, 20, 5)
        lines.append(f"whole step, t5-{a.t5} B={B}, train mode, host clock over 20 steps after 5: full fine-tuning with optim.FusedAdam {full:.2f} ms")
        del opt
    for targets in (("q", "v"), "all-linear"):
        for r in (8, 64):
            ad = lora.attach(m, r=r, alpha=2 * r, targets=targets)
            with torch.no_grad():
                for k, p in ad.named_parameters():
                    if ".lora_B." in k:
                        p.normal_(0.0, 0.01)
            m({"pixel_values": pix}, {"input_ids": src}, {"input_ids": tgt}).backward()  # leaves dW in the flat buffer
            eng, flat = m._engine, m.flat_grads("main")
            layout = eng.lora_layout()
            ws = [m.transformer.get_parameter(x + ".weight") for x in ad.modules]
            As = [p.data for k, p in ad.named_parameters() if ".lora_A." in k]
            Bs = [p.data for k, p in ad.named_parameters() if ".lora_B." in k]
            aoff = [layout[x + ".weight"][0] for x in ad.modules]
            goff = [layout[x + ".weight"][1] for x in ad.modules]
            n_el = sum(p.numel() for p in ws)
            arena = torch.empty(max(o + p.numel() for o, p in zip(aoff, ws)), dtype=torch.bfloat16, device="cuda")
            views = [arena[o:o + p.numel()].view(p.shape) for o, p in zip(aoff, ws)]
            dws = [flat[o:o + p.numel()].view(p.shape) for o, p in zip(goff, ws)]
            s = ad.scale

            def torch_merge():
                for v, p, A, Bm in zip(views, ws, As, Bs):
                    v.copy_(torch.addmm(p.data, Bm, A, alpha=s))

            def torch_grads():
                out = []
                for d, A, Bm in zip(dws, As, Bs):
                    out.append(torch.mm(Bm.t(), d).mul_(s))
                    out.append(torch.mm(d, A.t()).mul_(s))
                return out

            calls = {"a klab_lora_merge": lambda: ops.lora_merge(ad._desc, arena),
                     "b klab_lora_grads (2 launches)": lambda: eng.lora_grads(ad._out, ad._slab),
                     "c torch addmm + cast": torch_merge,
                     "d torch 2 x mm": torch_grads}
            dev = timed(calls, a.warm, a.n)
            n_ab = sum(p.numel() for p in As) + sum(p.numel() for p in Bs)
            slab = ad._slab.numel()
            floor = {"a": 6 * n_el + 4 * n_ab, "b": 4 * n_el + 8 * slab + 8 * n_ab, "c": 6 * n_el + 4 * n_ab, "d": 4 * n_el + 8 * n_ab}
            lines.append(f"LoRA kernels, t5-{a.t5}, targets {targets}, r = {r}: {len(ws)} tensors, {n_el} target elements, {n_ab} adapter elements, "
                         f"slab {slab} elements")
            lines.append(f"median (min) of {a.n} interleaved rounds (rotating order) after {a.warm} warm-up; device us between events behind a 10 ms "
                         f"product, caches flushed")
            lines.append(f"{'':32s} {'device us':>20s} {'bytes':>10s} {'GB/s':>7s} {'floor us':>9s} {'x floor':>8s}")
            for k in calls:
                nb = floor[k[0]]
                d, dm = statistics.median(dev[k]), min(dev[k])
                fl = nb / COPY_RATE * 1e6
                lines.append(f"{k:32s} {d:10.1f} ({dm:8.1f}) {nb / 1e6:8.1f}MB {nb / d / 1e3:7.0f} {fl:9.1f} {d / fl:8.2f}")
            if a.step:
                m._direct_grads = True
                opt = torch.optim.AdamW(ad.parameters(), lr=1e-3)
                t = step_time(m, batch, opt, 20, 5)
                lines.append(f"whole step with these adapters and torch.optim.AdamW: {t:.2f} ms ({ad.num_parameters()} trainable parameters)")
                del opt
            ad.detach()
            lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
