#!/usr/bin/env python3
"""Time of the cross-entropy with options on one MI355X at the BASELINE configs[1] logits (4096 rows x 32128 bf16: B = 64, Lt = 64,
the t5-small vocabulary), forward with d logits written in place, in one process:

  (a) plain            klab_ce_fwd: the existing kernel, the yardstick
  (b) opts neutral     klab_ce_fwd_opts with eps = 0, z = 0, no weights (the same bits as (a))
  (c) opts             klab_ce_fwd_opts with eps = 0.1, z = 1e-4, no weights
  (d) opts + weights   the same with per-row weights

Every call is the whole entry point: the counting (weight-sum) launch, the row kernel and the reduce.  The logits are restored
from a master copy before every timed call, outside the timed span (the kernels overwrite them with the gradient), followed by an
8192^2 fp32 product that pushes them out of the caches and keeps the device busy for ~10 ms, so the host has finished enqueueing
the call before the device reaches the first event -- the events bracket device time alone.  The four are interleaved in rounds
whose first form rotates.

Bytes: the row is read once and written once (the one-pass register form): 4 per logit, plus 8 + 4 per row for label and loss,
and 4 more per row with weights.  The spread of (a) is the range of its medians over consecutive blocks of ten rounds: what two
runs of the SAME kernel differ by.

    python tools/loss_options_bench.py [--out profiles/loss_options.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, V = 4096, 32128
EPS, Z = 0.1, 1e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_options_bench needs the GPU: nothing is measured without one")
    from klab_multimodalmodel_amd import ops
    g = torch.Generator().manual_seed(0)
    master = (3.0 * torch.randn(ROWS, V, generator=g)).to(torch.bfloat16).cuda()
    labels = torch.randint(0, V, (ROWS,), generator=g)
    labels[::17] = -100
    labels = labels.cuda()
    weights = torch.tensor([0.0, 0.25, 1.0, 3.0])[torch.randint(0, 4, (ROWS,), generator=g)].cuda()
    logits = torch.empty_like(master)
    inv, loss_row, loss = (torch.zeros(n, device="cuda") for n in (1, ROWS, 1))
    calls = {
        "a plain (yardstick)": lambda: ops.ce_fwd(logits, labels, inv, loss_row, loss, write_grad=True),
        "b opts, neutral": lambda: ops.ce_fwd_opts(logits, labels, None, inv, loss_row, loss, eps=0.0, z=0.0, write_grad=True),
        "c opts, eps + z": lambda: ops.ce_fwd_opts(logits, labels, None, inv, loss_row, loss, eps=EPS, z=Z, write_grad=True),
        "d opts, eps + z + w": lambda: ops.ce_fwd_opts(logits, labels, weights, inv, loss_row, loss, eps=EPS, z=Z, write_grad=True),
    }
    busy = torch.randn(8192, 8192, device="cuda")
    dev = {k: [] for k in calls}
    results = {}
    for r in range(a.warm + a.n):
        order = list(calls.items())
        order = order[r % len(order):] + order[:r % len(order)]  # every form takes every place in the round equally often
        for k, fn in order:
            logits.copy_(master)
            torch.mm(busy, busy)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warm:
                dev[k].append(e0.elapsed_time(e1) * 1e3)
            if r == 0:
                results[k] = (loss.clone(), logits.clone())
    same = all(torch.equal(results["a plain (yardstick)"][i], results["b opts, neutral"][i]) for i in (0, 1))
    lines = [f"cross-entropy forward + d logits in place, BASELINE configs[1] logits: {ROWS} rows x {V} bf16, {int((labels != -100).sum())} rows with a label",
             f"median (min) of {a.n} interleaved rounds (rotating order) after {a.warm} warm-up; device us between events behind a 10 ms product, "
             "logits restored and caches flushed before every call",
             f"{'':24s} {'device us':>18s} {'bytes':>10s} {'GB/s':>8s}"]
    for k in calls:
        nb = 4 * ROWS * V + (16 if k.startswith("d") else 12) * ROWS
        d, dm = statistics.median(dev[k]), min(dev[k])
        lines.append(f"{k:24s} {d:9.1f} ({dm:7.1f}) {nb / 1e6:8.1f}MB {nb / d / 1e3:8.0f}")
    ya = dev["a plain (yardstick)"]
    blocks = [statistics.median(ya[i:i + 10]) for i in range(0, a.n - 9, 10)]
    da, db, dc, dd = (statistics.median(dev[k]) for k in calls)
    lines.append(f"(a)'s medians over blocks of 10 rounds: {', '.join(f'{b:.1f}' for b in blocks)}: spread {max(blocks) - min(blocks):.1f} us")
    lines.append(f"(b) - (a) = {db - da:+.1f} us   (c) - (a) = {dc - da:+.1f} us   (d) - (a) = {dd - da:+.1f} us   (device medians)")
    lines.append(f"check: (b) equals (a) bit for bit in loss and d logits: {same};  losses a {float(results['a plain (yardstick)'][0]):.6f}  "
                 f"c {float(results['c opts, eps + z'][0]):.6f}  d {float(results['d opts, eps + z + w'][0]):.6f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not same:
        raise SystemExit("neutral options did not reproduce the plain kernel")


if __name__ == "__main__":
    main()
