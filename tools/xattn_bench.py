#!/usr/bin/env python3
"""What the cross-attention maps cost generate() on one MI355X: greedy generate at the BASELINE configs[1] shapes (Swin-V2 tiny +
T5-small, 224 x 224, bf16, batch 64, 9 source tokens, max_length 20) without and with return_cross_attention=True, in one process.

Per call the time between two stream events around generate() (the call reads one stop word per step, so this is the call as a
user sees it, host included).  Both forms are warmed up, then timed alternately --n times each; the output gives the median, the
minimum and the spread (10th to 90th percentile) of each, and the median of the per-pair differences.  The sequences of the two
forms are compared bit for bit before anything is timed, and min_new_tokens keeps every row generating to max_length so that both
forms run all 18 decoder steps whatever the random weights choose.

    python tools/xattn_bench.py [--n 30] [--batch 64] [--max-length 20]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--max-length", type=int, default=20)
    ap.add_argument("--dtype", default="bf16")
    a = ap.parse_args()
    from bench import synth_batch, workload_configs
    from klab_multimodalmodel_amd.models.model import MyModel
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    sw, t5 = workload_configs("caption")
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    torch.manual_seed(0)
    m = MyModel(args, _configs=(sw, t5, t5), _seed=0, dtype=a.dtype).to("cuda")
    pix, src, _ = synth_batch(a.batch, 9, 8, sw.image_size, 32128, "cuda")
    kw = dict(max_length=a.max_length, min_new_tokens=a.max_length - 1)

    def plain():
        return m.generate(pix, src, **kw)

    def maps():
        return m.generate(pix, src, return_cross_attention=True, **kw)

    seq, (seq2, info) = plain(), maps()
    assert torch.equal(seq, seq2) and seq.shape[1] == a.max_length
    att = info["cross_attention"]
    for _ in range(a.warm):
        plain()
        maps()
    times = {"plain": [], "maps": []}
    for _ in range(a.n):
        for name, fn in (("plain", plain), ("maps", maps)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    out = dict(shape=dict(batch=a.batch, max_length=a.max_length, dtype=a.dtype, maps=list(att.shape)), n=a.n)
    for name, t in times.items():
        q = statistics.quantiles(t, n=10)
        out[name] = dict(median_ms=round(statistics.median(t), 3), min_ms=round(min(t), 3), p10_ms=round(q[0], 3), p90_ms=round(q[-1], 3))
    out["median_pair_difference_ms"] = round(statistics.median(b - c for b, c in zip(times["maps"], times["plain"])), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
