#!/usr/bin/env python3
"""Training step with n captions per image on one MI355X at the headline configuration (bench.py's `caption` workload: Swin-V2
C=64 (2,2,6,2) 224 w7 frozen + T5-small, bf16, Ls = 9, Lt = 64, dropout on, klab FusedAdam), B = 64 images:

  grouped n    labels [B, n, Lt]: the Swin tower, the language encoder, the T5 encoder and its backward run once per image
  repeated n   the only form there was: the 2-D step on pixel_values / source ids repeat_interleave(n, 0) and labels [B*n, Lt]
  single       the 2-D step at B = 64 (n = 1), for scale

A step is forward + backward + optimizer.step() + zero_grad(), as bench.py times it.  All forms live in one process, each with its
own model and binding; they are timed interleaved: one round runs every form once (`--chunk` steps back to back between two HIP
events, the device idle before the first), the first form of a round rotates, and a form's figure is the median over the rounds of
its chunk time / chunk.  The spread of a form is the range of its medians over consecutive blocks of five rounds -- what two
measurements of the SAME form differ by; a difference between forms below that is not a difference.

Memory: bytes of the engine's workspace of each binding, and the process's peak allocation while that form alone warms up (weights,
gradients, optimizer state, inputs and workspace), from torch's allocator.

    python tools/multi_caption_bench.py [--n 2 5] [--out profiles/multi_caption.txt]
"""
import argparse
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Form:
    def __init__(self, name, images, captions, grouped, wl, sw, t5, dev):
        from bench import synth_batch
        from klab_multimodalmodel_amd.models.model import MyModel
        from klab_multimodalmodel_amd.optim import FusedAdam
        self.name, self.images, self.captions = name, images, captions
        args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=wl["train_swin"],
                                     transformer_model_name="-")
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        torch.manual_seed(0)
        self.model = MyModel(args, _configs=(sw, t5, t5), _seed=0, dtype="bf16").to(dev)
        self.model._direct_grads = True
        self.model.transformer.train()
        self.opt = FusedAdam(self.model.transformer.parameters(), lr=1e-3)
        # the same images, prompts and captions in both forms: the grouped labels viewed [B*n, Lt] are the repeated form's
        pix, src, _ = synth_batch(images, wl["Ls"], wl["Lt"], sw.image_size, 32128, dev)
        _, _, tgt = synth_batch(images * captions, wl["Ls"], wl["Lt"], sw.image_size, 32128, dev, seed=4321)
        if grouped:
            tgt = tgt.view(images, captions, wl["Lt"])
        elif captions > 1:
            pix, src = pix.repeat_interleave(captions, 0).contiguous(), src.repeat_interleave(captions, 0).contiguous()
        self.batch = ({"pixel_values": pix}, {"input_ids": src}, {"input_ids": tgt})
        for _ in range(3):
            self.loss = self.step()
        torch.cuda.synchronize()
        self.peak = torch.cuda.max_memory_allocated() - base
        self.workspace = self.model._engine.workspace.numel()
        self.ms = []

    def step(self):
        loss = self.model(*self.batch)
        loss.backward()
        self.opt.step()
        self.opt.zero_grad()
        return loss

    def timed(self, chunk):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(chunk):
            self.step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / chunk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2, 5])
    ap.add_argument("--batch", type=int, default=64, help="images per step")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3, help="rounds thrown away")
    ap.add_argument("--chunk", type=int, default=5, help="steps per timed span")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multi_caption_bench needs the GPU: nothing is measured without one")
    from bench import WORKLOADS, workload_configs
    wl = WORKLOADS["caption"]
    sw, t5 = workload_configs("caption")
    dev = torch.device("cuda", 0)
    B = a.batch
    forms = [Form("single (2-D, n = 1)", B, 1, False, wl, sw, t5, dev)]
    for n in a.n:
        forms.append(Form(f"grouped n = {n}", B, n, True, wl, sw, t5, dev))
        forms.append(Form(f"repeated n = {n}", B, n, False, wl, sw, t5, dev))
    for r in range(a.warm + a.rounds):
        order = forms[r % len(forms):] + forms[:r % len(forms)]
        for f in order:
            t = f.timed(a.chunk)
            if r >= a.warm:
                f.ms.append(t)
    lines = [f"training step with n captions per image, {wl['name']}, bf16, B = {B} images, Ls = {wl['Ls']}, Lt = {wl['Lt']}, dropout on, FusedAdam",
             f"median (min) over {a.rounds} interleaved rounds of {a.chunk} steps (rotating order) after {a.warm} warm-up rounds; spread = range of "
             "the medians over blocks of five rounds",
             f"{'':22s} {'ms / step':>18s} {'spread':>8s} {'captions/s':>11s} {'workspace':>10s} {'peak alloc':>11s} {'loss':>8s}"]
    med = {}
    for f in forms:
        m, lo = statistics.median(f.ms), min(f.ms)
        blocks = [statistics.median(f.ms[i:i + 5]) for i in range(0, len(f.ms) - 4, 5)]
        med[f.name] = m
        lines.append(f"{f.name:22s} {m:9.3f} ({lo:7.3f}) {max(blocks) - min(blocks):8.3f} {f.images * f.captions / m * 1e3:11.0f} "
                     f"{f.workspace / 2 ** 30:8.2f}Gi {f.peak / 2 ** 30:9.2f}Gi {float(f.loss.detach()):8.4f}")
    single = med["single (2-D, n = 1)"]
    for n in a.n:
        g, rp = med[f"grouped n = {n}"], med[f"repeated n = {n}"]
        lines.append(f"n = {n}: grouped / repeated = {g / rp:.3f} ({rp - g:+.3f} ms saved per step, {(rp - g) / (n - 1):.3f} ms per caption spared its "
                     f"encoder side; the single step takes {single:.3f} ms)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
