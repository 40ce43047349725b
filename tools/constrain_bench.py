#!/usr/bin/env python3
"""What trie-constrained decoding costs on one MI355X, in one process and one run:

  1. the host build of the trie (constrain.TokenTrie.from_sequences) for 1000 and for 100 000 random phrases of 1 to 8 tokens
  2. klab_constrain_rows at 64 and 320 rows, V = 32128, bf16 logits in and f32 rows out, for both tries with every row at the
     root and with every row at a deep node: device us between events behind a ~10 ms product (so the events bracket device
     time alone), median (min) of --n rounds; beside it, in the same rounds, klab_logits_process_rows with neutral settings and
     `out` written (the same row traffic without a trie), and the byte floor rows x V x 6 B at the achievable HBM rate
  3. the per-step time of a greedy session at B = 64, max_length 20 on bench.py's caption model (bf16): plain, and constrained
     to the 1000-phrase trie whose phrases are long enough that no row ends early (host wall time of the whole generate call
     over its positions, median of --n calls)

    python tools/constrain_bench.py [--out profiles/constrain.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, EOS = 32128, 1
HBM_GBS = 6300.0  # what a float4 copy reaches on this part (8 TB/s spec); the floor below is bytes / this rate


def phrases(rng, count, lo=1, hi=8):
    """`count` id lists of lo .. hi ids >= 2; the first token from 200 values and the second from 2000, so the root is wide and the
    deeper nodes narrow, as class names are"""
    lens = rng.integers(lo, hi + 1, count)
    out = []
    for n in lens:
        p = [int(rng.integers(2, 202))] + ([int(rng.integers(2, 2002))] if n > 1 else []) + rng.integers(2, V, max(0, n - 2)).tolist()
        out.append(p)
    return out


def med(v):
    return f"{statistics.median(v):8.1f} ({min(v):7.1f})"


def kernel_lines(a, tries):
    from klab_multimodalmodel_amd import _lib as L
    lib = L.load()
    lines = []
    busy = torch.randn(8192, 8192, device="cuda")
    for rows in (64, 320):
        x = (torch.randn(rows, V, device="cuda") * 3.0).to(torch.bfloat16)
        out = torch.empty(rows, V, device="cuda")
        seq = torch.zeros(rows, 2, dtype=torch.int64, device="cuda")
        p = L.LogitsProcArgs()
        p.dtype, p.logits, p.ld, p.row_div, p.rows, p.V = L.BF16, x.data_ptr(), V, 1, rows, V
        p.seq, p.ld_seq, p.cur_len, p.repetition_penalty, p.eos_id, p.out, p.ld_out = seq.data_ptr(), 2, 1, 1.0, EOS, out.data_ptr(), V
        calls = {"klab_logits_process_rows": lambda: lib.klab_logits_process_rows(C.byref(p), L.stream_ptr())}
        keep = []
        for name, (trie, deep) in tries.items():
            for where, node in (("root", int(trie.roots[0])), ("deep node", deep)):
                # a row reaches `node` by an advance over the edge that leads to it
                par = int((trie.child_node.cpu() == node).nonzero()[0]) if where != "root" else -1
                off = trie.child_off.cpu()
                src = int(torch.searchsorted(off, torch.tensor(par), right=True)) - 1 if par >= 0 else 0
                tok = int(trie.child_tok[par]) if par >= 0 else 0
                nin = torch.full((rows,), src, dtype=torch.int32, device="cuda")
                last = torch.full((rows,), tok, dtype=torch.int64, device="cuda")
                nout = torch.empty(rows, dtype=torch.int32, device="cuda")
                roots = trie.roots[:1].repeat(rows).contiguous()
                c = L.ConstrainArgs()
                c.dtype, c.logits, c.ld, c.row_div, c.rows, c.V = L.BF16, x.data_ptr(), V, 1, rows, V
                c.child_off, c.child_tok, c.child_node = trie.child_off.data_ptr(), trie.child_tok.data_ptr(), trie.child_node.data_ptr()
                c.n_nodes, c.n_edges, c.first, c.root, c.root_div = trie.n_nodes, trie.n_edges, int(par < 0), roots.data_ptr(), 1
                c.node_in, c.last_tok, c.node_out, c.eos_id, c.out, c.ld_out = nin.data_ptr(), last.data_ptr(), nout.data_ptr(), EOS, out.data_ptr(), V
                keep.append((c, nin, last, nout, roots))
                deg = int(off[node + 1] - off[node])
                calls[f"{name}, {where} ({deg} children)"] = lambda c=c: lib.klab_constrain_rows(C.byref(c), L.stream_ptr())
        dev = {k: [] for k in calls}
        for r in range(a.warm + a.n):
            for k, fn in calls.items():
                torch.mm(busy, busy)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn()
                e1.record()
                torch.cuda.synchronize()
                assert rc == 0, (k, rc)
                if r >= a.warm:
                    dev[k].append(e0.elapsed_time(e1) * 1e3)
        floor = rows * V * 6 / (HBM_GBS * 1e3)
        lines.append(f"  {rows} rows: byte floor rows x V x 6 B = {rows * V * 6 / 2 ** 20:.1f} MiB, {floor:.1f} us at {HBM_GBS / 1e3:.1f} TB/s")
        for k, v in dev.items():
            lines.append(f"    {k:48s} {med(v)} us")
    return lines


def session_lines(a, trie):
    import bench
    from klab_multimodalmodel_amd.models.model import MyModel
    sw, t5 = bench.cfg2_configs()
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _seed=0, dtype="bf16").to("cuda")
    gen = torch.Generator().manual_seed(0)
    B, Lm = 64, 20
    pix = torch.randn(B, 3, sw.image_size, sw.image_size, generator=gen).cuda()
    src = torch.randint(2, t5.vocab_size, (B, 16), generator=gen).cuda()
    t = {}
    for name, kw in (("plain", dict(min_length=Lm)), ("constrained", dict(constraint=trie))):
        ts, steps = [], 0
        for r in range(a.warm + a.n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.generate(pix, src, max_length=Lm, **kw)
            torch.cuda.synchronize()
            if r >= a.warm:
                ts.append((time.perf_counter() - t0) * 1e3)
            steps = out.shape[1] - 1
        t[name] = (statistics.median(ts), min(ts), steps)
    lines = [f"greedy session at B = {B}, max_length {Lm}, bf16, bench.py's caption model: host wall ms of one generate call (prefill + "
             f"every position), median (min) of {a.n} calls"]
    for name, (md, mn, steps) in t.items():
        lines.append(f"  {name:12s} {md:8.2f} ({mn:8.2f}) ms over {steps} positions")
    (p, _, sp), (c, _, sc) = t["plain"], t["constrained"]
    lines.append(f"  per position: {(c - p) / max(sc, 1) * 1e3:.1f} us more with the constraint ({sc} positions against {sp}; the plain session "
                 f"holds EOS back with min_length so that both run to max_length)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrain.txt"))
    a = ap.parse_args()
    from klab_multimodalmodel_amd.constrain import TokenTrie
    rng = np.random.default_rng(0)
    lines, tries = ["host build of the trie (constrain.TokenTrie.from_sequences, numpy, one pass per depth), wall ms"], {}
    for count in (1000, 100_000):
        ps = phrases(rng, count)
        t0 = time.perf_counter()
        trie = TokenTrie.from_sequences(ps, V, EOS)
        ms = (time.perf_counter() - t0) * 1e3
        lines.append(f"  {count:7d} phrases: {ms:8.1f} ms -> {trie.n_nodes} nodes, {trie.n_edges} edges ({(trie.n_nodes + 1 + 2 * trie.n_edges) * 4 / 2 ** 20:.2f} MiB)")
        trie.to("cuda")
        deep = trie.walk(max(ps, key=len)[:-1])
        tries[f"{count}-phrase trie"] = (trie, deep)
    lines.append("")
    lines.append(f"klab_constrain_rows, V = {V}, bf16 in, f32 out; device us between events behind a 10 ms product, median (min) of {a.n} rounds "
                 f"after {a.warm} warm-up; klab_logits_process_rows: neutral settings, out written, same rounds")
    lines += kernel_lines(a, tries)
    lines.append("")
    long_trie = TokenTrie.from_sequences(phrases(rng, 1000, 19, 19), V, EOS).to("cuda")
    lines += session_lines(a, long_trie)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
