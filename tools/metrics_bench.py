#!/usr/bin/env python3
"""What the caption-metric statistics cost on one MI355X, in one process and one run:

  1. klab_caption_stats at B = 64 images, R = 5 references, L = 20 (Lr = 16) with n = 1 and n = 5 hypotheses per image, and at the
     limits (B = 64, n = 5, R = 16 references of 64 units, L = 65): device us between events behind a ~10 ms product (so the events
     bracket device time alone), median (min) of --n rounds
  2. klab_ciderd_rewards on the same inputs, beside each row
  3. the host round trip the kernel replaces: the sequences copied to the host and the Python reference of tests/metrics_ref.py
     over the B * n captions, nothing copied back (host wall time, one round)

    python tools/metrics_bench.py [--out profiles/metrics.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.scst_bench import EOS, V, corpus, zipf_captions  # noqa: E402  (the same synthetic captions as the rewards' measurement)

B = 64


def med(v):
    return f"{statistics.median(v):9.1f} ({min(v):7.1f})"


def inputs(rng, corp, n, R, L, Lr, lo, hi):
    """refs [B, R, Lr] of EOS-closed captions of lo..hi tokens and hyp [B * n, L]: half a reference of the image, half fresh tokens"""
    refs = torch.full((B, R, Lr), -100, dtype=torch.int64)
    caps = zipf_captions(rng, B * R)
    for b in range(B):
        for j in range(R):
            own = corp[b][j % len(corp[b])][:-1]
            cap = (own + caps[b * R + j][:-1] * 24)[:int(rng.integers(lo, hi + 1))] + [EOS]
            refs[b, j, :len(cap)] = torch.tensor(cap)
    hyp = torch.zeros(B * n, L, dtype=torch.int64)
    for r, cap in enumerate(zipf_captions(rng, B * n)):
        own = refs[r // n, r % R].tolist()
        own = own[:own.index(EOS)]
        cap = (own[:len(own) // 2] + cap[:-1] * 24)[:min(L - 2, int(rng.integers(lo, hi + 1)))] + [EOS]
        hyp[r, 1:1 + len(cap)] = torch.tensor(cap)
    return hyp, refs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs the GPU: nothing is measured without one")
    from klab_multimodalmodel_amd import metrics, ops, scst
    from tests import metrics_ref as M
    rng = np.random.default_rng(0)
    corp = corpus(rng, 2000)
    table = scst.CiderD.from_references(corp, vocab_size=V, eos_token_id=EOS).to("cuda")
    shapes = {"n = 1": (1, 5, 20, 16, 6, 14), "n = 5": (5, 5, 20, 16, 6, 14), "limits": (5, 16, 65, 64, 63, 63)}
    data, calls = {}, {}
    for name, (n, R, L, Lr, lo, hi) in shapes.items():
        hyp, refs = inputs(rng, corp, n, R, L, Lr, lo, hi)
        hd, rd = hyp.cuda(), refs.cuda()
        st, rew = torch.empty(B * n, 16, dtype=torch.int32, device="cuda"), torch.empty(B * n, device="cuda")
        data[name] = (hyp, refs, n, st)
        calls[name, "stats"] = lambda hd=hd, rd=rd, st=st, n=n: ops.caption_stats(hd, rd, st, n_h=n, eos=EOS, count_eos=False)
        calls[name, "rewards"] = lambda hd=hd, rd=rd, rew=rew, n=n: ops.ciderd_rewards(hd, rd, table.keys, table.idf, table.log_n, rew, n_h=n,
                                                                                      eos=EOS)
    busy = torch.randn(8192, 8192, device="cuda")
    dev = {k: [] for k in calls}
    for r in range(a.warm + a.n):
        for k, fn in calls.items():
            torch.mm(busy, busy)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warm:
                dev[k].append(e0.elapsed_time(e1) * 1e3)
    # the round trip the kernel replaces, and the integers it has to give
    host = {}
    for name, (hyp, refs, n, st) in data.items():
        hd = hyp.cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_hyp = hd.cpu()
        t1 = time.perf_counter()
        want = M.stats(host_hyp, refs, n, EOS, False)
        t2 = time.perf_counter()
        host[name] = (1e3 * (t1 - t0), 1e3 * (t2 - t1), bool(torch.equal(st.cpu(), want)))
    hyp, refs, n, st = data["n = 5"]
    sc = metrics.sentence_scores(st).view(-1, 5).mean(0).tolist()
    lines = [f"caption-metric statistics at B = {B} images; captions of the rewards' measurement (tools/scst_bench.py), half a reference "
             "and half fresh tokens",
             f"device us between events behind a 10 ms product, median (min) of {a.n} rounds after {a.warm} warm-up; "
             f"one launch of {B} workgroups of 512 threads each",
             "                                           klab_caption_stats       klab_ciderd_rewards"]
    for name, (n, R, L, Lr, lo, hi) in shapes.items():
        lines.append(f"  {name:7s} R = {R:2d}, L = {L:2d}, Lr = {Lr:2d}, {lo}..{hi} units   {med(dev[name, 'stats'])} us   {med(dev[name, 'rewards'])} us")
    lines.append("the host round trip the kernel replaces (host wall, once): sequences to the host, then the Python reference "
                 "(Counter n-grams, LCS table), nothing back")
    for name, (n, R, L, Lr, lo, hi) in shapes.items():
        cp, py, same = host[name]
        lines.append(f"  {name:7s} {B * n:4d} captions   copy {cp:7.3f} ms   reference {py:9.1f} ms   kernel integers "
                     f"{'equal' if same else 'DIFFER FROM'} the reference")
    lines.append("mean sentence scores at n = 5: " + ", ".join(f"{k} {v:.4f}" for k, v in zip(metrics.SCORES, sc)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not all(h[2] for h in host.values()):
        raise SystemExit("the kernel's integers differ from the reference")


if __name__ == "__main__":
    main()
