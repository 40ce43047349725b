#!/usr/bin/env python3
"""Time of the cross-entropy with knowledge distillation on one MI355X at the BASELINE configs[1] logits (4096 rows x 32128 bf16:
B = 64, Lt = 64, the t5-small vocabulary), forward with d logits written in place, in one process and one run:

  (a) plain              klab_ce_fwd: the existing kernel
  (b) opts               klab_ce_fwd_opts, neutral options: the yardstick
  (c) distill bf16 T=1   klab_ce_fwd_distill, alpha = 0.5, bf16 teacher
  (d) distill bf16 T=2
  (e) distill f32  T=1   the same with an fp32 teacher
  (f) distill f32  T=2
  (g) two launches T=2   klab_ce_fwd_opts on the logits plus the soft term ALONE on a second copy of them (klab_ce_fwd_distill at
                         alpha = 1, bf16 teacher): a lower bound of any two-launch statement of the loss -- the pass that would add
                         the two gradients (three more streams) is left out

Method and table are tools/loss_options_bench.py's: every call is the whole entry point (weight sum, row kernel, reduce); the logits
are restored before every timed call outside the timed span, followed by an 8192^2 fp32 product that pushes them out of the caches
and keeps the device busy for ~10 ms, so the events bracket device time alone; the forms are interleaved in rounds whose first
form rotates.  Byte floor: student read + student written + teacher read (2 + 2 + 2 or 4 bytes per logit).

With --step also one T5-small training step (bench.py's caption workload: B = 64, FusedAdam, train mode) plain against distilled
with the teacher's logits pre-computed (a fixed bf16 tensor), interleaved, host wall time per step with a synchronize.

    python tools/distill_bench.py [--step] [--out profiles/distill.txt]
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

ROWS, V = 4096, 32128
ALPHA = 0.5


def kernel_table(a):
    from klab_multimodalmodel_amd import ops
    g = torch.Generator().manual_seed(0)
    master = (3.0 * torch.randn(ROWS, V, generator=g)).to(torch.bfloat16).cuda()
    t32 = (0.7 * master.float() + 2.0 * torch.randn(ROWS, V, generator=g).cuda())
    t16 = t32.to(torch.bfloat16)
    labels = torch.randint(0, V, (ROWS,), generator=g)
    labels[::17] = -100
    labels = labels.cuda()
    logits, second = torch.empty_like(master), torch.empty_like(master)
    inv, loss_row, kl_row, loss, loss2 = (torch.zeros(n, device="cuda") for n in (1, ROWS, ROWS, 1, 1))

    def distill(teacher, T, alpha=ALPHA, x=None, out=None):
        return lambda: ops.ce_fwd_distill(logits if x is None else x, teacher, labels, None, inv, loss_row, kl_row, loss if out is None else out,
                                          alpha=alpha, temperature=T, write_grad=True)

    def two():
        ops.ce_fwd_opts(logits, labels, None, inv, loss_row, loss, write_grad=True)
        distill(t16, 2.0, 1.0, second, loss2)()

    calls = {
        "a plain": lambda: ops.ce_fwd(logits, labels, inv, loss_row, loss, write_grad=True),
        "b opts (yardstick)": lambda: ops.ce_fwd_opts(logits, labels, None, inv, loss_row, loss, eps=0.0, z=0.0, write_grad=True),
        "c distill bf16 T=1": distill(t16, 1.0),
        "d distill bf16 T=2": distill(t16, 2.0),
        "e distill f32  T=1": distill(t32, 1.0),
        "f distill f32  T=2": distill(t32, 2.0),
        "g two launches T=2": two,
    }
    busy = torch.randn(8192, 8192, device="cuda")
    dev = {k: [] for k in calls}
    first = {}
    for r in range(a.warm + a.n):
        order = list(calls.items())
        order = order[r % len(order):] + order[:r % len(order)]
        for k, fn in order:
            logits.copy_(master)
            second.copy_(master)
            torch.mm(busy, busy)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warm:
                dev[k].append(e0.elapsed_time(e1) * 1e3)
            if r == 0:
                first[k] = float(loss)
    lines = [f"cross-entropy + distillation forward + d logits in place, BASELINE configs[1] logits: {ROWS} rows x {V} bf16, alpha = {ALPHA}",
             f"median (min) of {a.n} interleaved rounds (rotating order) after {a.warm} warm-up; device us between events behind a 10 ms product, "
             "logits restored and caches flushed before every call",
             f"{'':22s} {'device us':>18s} {'floor bytes':>12s} {'GB/s':>8s} {'exp / logit':>12s} {'loss':>10s}"]
    streams = {"a": 4, "b": 4, "c": 6, "d": 6, "e": 8, "f": 8, "g": 10}
    exps = {"a": 2, "b": 2, "c": 4, "d": 6, "e": 4, "f": 6, "g": 8}
    for k in calls:
        nb = streams[k[0]] * ROWS * V
        d, dm = statistics.median(dev[k]), min(dev[k])
        lines.append(f"{k:22s} {d:9.1f} ({dm:7.1f}) {nb / 1e6:10.1f}MB {nb / d / 1e3:8.0f} {exps[k[0]]:12d} {first[k]:10.5f}")
    yb = dev["b opts (yardstick)"]
    blocks = [statistics.median(yb[i:i + 10]) for i in range(0, a.n - 9, 10)]
    lines.append(f"(b)'s medians over blocks of 10 rounds: {', '.join(f'{b:.1f}' for b in blocks)}: spread {max(blocks) - min(blocks):.1f} us")
    med = {k[0]: statistics.median(v) for k, v in dev.items()}
    lines.append("ratio to (b): " + "  ".join(f"({c}) {med[c] / med['b']:.2f}" for c in "cdefg"))
    lines.append(f"one launch against two at T = 2, bf16 teacher: (d) {med['d']:.1f} us, (g) {med['g']:.1f} us "
                 "(g leaves out the pass that adds the two gradients)")
    return lines


def step_rows(a):
    import bench
    from klab_multimodalmodel_amd.models.model import MyModel
    from klab_multimodalmodel_amd.optim import FusedAdam
    wl = bench.WORKLOADS["caption"]
    sw, t5 = bench.workload_configs("caption")
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=wl["train_swin"],
                                 transformer_model_name="-")
    torch.manual_seed(0)
    m = MyModel(args, _configs=(sw, t5, t5), _seed=0, dtype="bf16").to("cuda")
    m._direct_grads = True
    opt = FusedAdam(m.transformer.parameters(), lr=1e-3)
    m.transformer.train()
    B, Ls, Lt = wl["B"], wl["Ls"], wl["Lt"]
    pix, src, tgt = bench.synth_batch(B, Ls, Lt, sw.image_size, 32128, torch.device("cuda"), seed=1234)
    teacher = (2.0 * torch.randn(B, Lt, t5.vocab_size, device="cuda")).to(torch.bfloat16)
    images, se = {"pixel_values": pix}, {"input_ids": src}

    def step(distilled, T=2.0):
        m.set_loss_options(distill_alpha=ALPHA if distilled else 0.0, distill_temperature=T)
        te = {"input_ids": tgt, "teacher_logits": teacher} if distilled else {"input_ids": tgt}
        loss = m(images, se, te)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss

    forms = {"plain step": lambda: step(False), "distilled step T=1": lambda: step(True, 1.0), "distilled step T=2": lambda: step(True, 2.0)}
    wall = {k: [] for k in forms}
    for r in range(a.warm + a.n):
        order = list(forms.items())
        order = order[r % len(order):] + order[:r % len(order)]
        for k, fn in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= a.warm:
                wall[k].append((time.perf_counter() - t0) * 1e3)
    lines = [f"one T5-small training step, bench.py's caption workload (B = {B}, Lt = {Lt}, bf16, FusedAdam, train mode), teacher logits "
             f"pre-computed (bf16 [{B}, {Lt}, {t5.vocab_size}]): host wall ms per step with a synchronize, median (min) of {a.n} interleaved rounds"]
    for k in forms:
        lines.append(f"{k:22s} {statistics.median(wall[k]):8.3f} ({min(wall[k]):8.3f}) ms")
    p = statistics.median(wall["plain step"])
    lines.append("distilled - plain: " + "  ".join(f"{k[-3:]} {statistics.median(wall[k]) - p:+.3f} ms" for k in forms if k != "plain step"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--step", action="store_true", help="also time one T5-small training step plain against distilled")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_bench needs the GPU: nothing is measured without one")
    lines = kernel_table(a)
    if a.step:
        torch.cuda.empty_cache()
        lines += [""] + step_rows(a)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
