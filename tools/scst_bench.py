#!/usr/bin/env python3
"""What self-critical training costs on one MI355X, in one process and one run:

  1. klab_ciderd_rewards and klab_scst_targets at B = 64 images, n = 5 samples, R = 5 references, L = 20: device us between events
     behind a ~10 ms product (so the events bracket device time alone), median (min) of --n rounds; the rewards kernel with the
     table of a 2000-image corpus and with the COCO-sized table of 2.; beside the rewards kernel what
     it replaces: the sequences copied to the host, the fp64 Python reference of tests/scst_ref.py over the B * n captions, the
     rewards copied back (host wall time, one round)
  2. the host build of the idf table (scst.CiderD.from_references) for a synthetic COCO-sized corpus: --corpus-images images x 5
     references of about 11 tokens from a Zipf-like vocabulary
  3. with --step: one self-critical step (scst.SelfCritical, greedy baseline, 5 samples, max_length 20) beside the cross-entropy
     step of bench.py's caption workload (B = 64, Lt = 64, bf16, FusedAdam, train mode): host wall ms with a synchronize per phase
     -- sampling session, greedy session, rewards + targets, forward + backward + optimizer -- and the re-binding alone (the engine
     bound back and forth between the session's and the training forward's shapes, nothing else run)

    python tools/scst_bench.py [--step] [--out profiles/scst.txt]
"""
import argparse
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N, R, L, LR = 64, 5, 5, 20, 16
V, EOS = 32128, 1


def zipf_captions(rng, count, mean_len=11):
    """`count` EOS-closed id lists of about mean_len tokens, ids 2 .. V - 1 with frequency ~ 1 / rank"""
    lens = np.clip(rng.poisson(mean_len - 1, count), 4, LR - 1)
    ranks = np.minimum((np.exp(rng.uniform(0.0, np.log(V - 2), int(lens.sum())))).astype(np.int64) + 1, V - 1)
    out, at = [], 0
    for n in lens:
        out.append(ranks[at:at + n].tolist() + [EOS])
        at += n
    return out


def corpus(rng, images):
    caps = zipf_captions(rng, images * R)
    return [caps[i * R:(i + 1) * R] for i in range(images)]


def med(v):
    return f"{statistics.median(v):9.1f} ({min(v):7.1f})"


def kernel_rows(a, big):
    from klab_multimodalmodel_amd import ops, scst
    from tests import scst_ref as S
    rng = np.random.default_rng(0)
    corp = corpus(rng, 2000)
    table = scst.CiderD.from_references(corp, vocab_size=V, eos_token_id=EOS).to("cuda")
    refs = torch.full((B, R, LR), -100, dtype=torch.int64)
    for b in range(B):
        for j, cap in enumerate(corp[b]):
            refs[b, j, :len(cap)] = torch.tensor(cap)
    hyp = torch.zeros(B * N, L, dtype=torch.int64)
    for r, cap in enumerate(zipf_captions(rng, B * N)):
        own = corp[r // N][r % R]  # half a reference of the image, half fresh tokens: rewards of every size
        cap = (own[:len(own) // 2] + cap)[:L - 2] + [EOS]
        hyp[r, 1:1 + len(cap)] = torch.tensor(cap)
    hyp_d, refs_d = hyp.cuda(), refs.cuda()
    rew, rew2, base = torch.empty(B * N, device="cuda"), torch.empty(B * N, device="cuda"), torch.rand(B, device="cuda")
    big = big.to("cuda")
    labels = torch.empty(B, N, L - 1, dtype=torch.int64, device="cuda")
    weights, adv = torch.empty(B, N, L - 1, device="cuda"), torch.empty(B, N, device="cuda")
    calls = {
        "klab_ciderd_rewards": lambda: ops.ciderd_rewards(hyp_d, refs_d, table.keys, table.idf, table.log_n, rew, n_h=N, eos=EOS),
        "rewards, large table": lambda: ops.ciderd_rewards(hyp_d, refs_d, big.keys, big.idf, big.log_n, rew2, n_h=N, eos=EOS),
        "klab_scst_targets": lambda: ops.scst_targets(hyp_d, rew, base, labels, weights, adv, n=N, mode=0, eos=EOS),
    }
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
    # the round trip the kernel replaces
    df = S.doc_freq(corp, EOS, True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_hyp = hyp_d.cpu()
    t1 = time.perf_counter()
    want = S.rewards(host_hyp, refs, N, df, len(corp), EOS, True)
    t2 = time.perf_counter()
    back = torch.from_numpy(want).float().cuda()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    err = float((rew.double().cpu() - torch.from_numpy(want)).abs().max())
    lines = [f"self-critical kernels at B = {B} images, n = {N} samples, R = {R} references, L = {L} (Lr = {LR}); table of {table.entries} "
             f"n-grams in {table.capacity} slots from a 2000-image corpus",
             f"device us between events behind a 10 ms product, median (min) of {a.n} rounds after {a.warm} warm-up",
             f"  klab_ciderd_rewards   {med(dev['klab_ciderd_rewards'])} us   one launch, {B} workgroups of 512 threads",
             f"  ... COCO-sized table  {med(dev['rewards, large table'])} us   the same launch probing {big.capacity} slots "
             f"({big.capacity * 12 / 2 ** 20:.0f} MiB: not cache-resident)",
             f"  klab_scst_targets     {med(dev['klab_scst_targets'])} us   one launch, {(B * N + 3) // 4} workgroups of 256 threads",
             f"the host round trip the rewards kernel replaces (host wall, once): sequences to the host {1e3 * (t1 - t0):.3f} ms, "
             f"fp64 Python CIDEr-D over {B * N} captions {1e3 * (t2 - t1):.1f} ms, rewards back {1e3 * (t3 - t2):.3f} ms",
             f"rewards: mean {float(rew.mean()):.3f}, max {float(rew.max()):.3f}; largest |kernel - fp64 reference| {err:.2e}"]
    del back
    return lines


def table_rows(a):
    from klab_multimodalmodel_amd import scst
    rng = np.random.default_rng(1)
    corp = corpus(rng, a.corpus_images)
    t0 = time.perf_counter()
    table = scst.CiderD.from_references(corp, vocab_size=V, eos_token_id=EOS)
    dt = time.perf_counter() - t0
    return table, [f"idf table of a synthetic COCO-sized corpus ({a.corpus_images} images x {R} references of about 11 tokens): "
            f"CiderD.from_references {dt:.1f} s on the host, {table.entries} n-grams in {table.capacity} slots "
            f"({table.capacity * 12 / 2 ** 20:.0f} MiB on the device)"]


def step_rows(a):
    import bench
    from klab_multimodalmodel_amd import ops, scst
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
    Bw, Ls, Lt = wl["B"], wl["Ls"], wl["Lt"]
    pix, src, tgt = bench.synth_batch(Bw, Ls, Lt, sw.image_size, 32128, torch.device("cuda"), seed=1234)
    images, se = {"pixel_values": pix}, {"input_ids": src}
    rng = np.random.default_rng(2)
    corp = corpus(rng, 2000)
    table = scst.CiderD.from_references(corp, vocab_size=t5.vocab_size, eos_token_id=t5.eos_token_id).to("cuda")
    refs = torch.full((Bw, R, LR), -100, dtype=torch.int64)
    for b in range(Bw):
        for j, cap in enumerate(corp[b]):
            refs[b, j, :len(cap)] = torch.tensor(cap)
    refs = refs.cuda()
    sc = scst.SelfCritical(m, table, samples=N, baseline="greedy", max_length=L)
    eos = t5.eos_token_id

    def tick():
        torch.cuda.synchronize()
        return time.perf_counter()

    def ce_step():
        t0 = tick()
        loss = m(images, se, {"input_ids": tgt})
        loss.backward()
        opt.step()
        opt.zero_grad()
        return {"step": tick() - t0}

    def scst_whole():
        t0 = tick()
        loss, _info = sc.loss(images, se, refs)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return {"step": tick() - t0}

    def scst_phases():  # SelfCritical.loss by hand, a synchronize between its phases
        out = {}
        t0 = tick()
        m.transformer.eval()
        seq = m.generate(pix, src, max_length=L, do_sample=True, num_return_sequences=N, top_k=0)
        t1 = tick()
        greedy = m.generate(pix, src, max_length=L)
        m.transformer.train()
        t2 = tick()
        rew, base = torch.empty(Bw * N, device="cuda"), torch.empty(Bw, device="cuda")
        ops.ciderd_rewards(seq, refs, table.keys, table.idf, table.log_n, rew, n_h=N, eos=eos)
        ops.ciderd_rewards(greedy, refs, table.keys, table.idf, table.log_n, base, n_h=1, eos=eos)
        labels = torch.empty(Bw, N, L - 1, dtype=torch.int64, device="cuda")
        weights, adv = torch.empty(Bw, N, L - 1, device="cuda"), torch.empty(Bw, N, device="cuda")
        ops.scst_targets(seq, rew, base, labels, weights, adv, n=N, mode=0, eos=eos)
        t3 = tick()
        m.set_loss_options(weight_norm="count")
        loss = m(images, se, {"input_ids": labels, "loss_weights": weights})
        loss.backward()
        opt.step()
        opt.zero_grad()
        m.set_loss_options()
        t4 = tick()
        out.update(sampling=t1 - t0, greedy=t2 - t1, rewards_targets=t3 - t2, fwd_bwd_opt=t4 - t3, step=t4 - t0)
        return out

    def rebind():  # the two re-bindings of a step, alone: the session's shape, then the training forward's
        t0 = tick()
        m._engine_for(pix, src, torch.empty(Bw, L - 1, dtype=torch.int64, device="cuda"))
        t1 = tick()
        m._engine_for(pix, src, torch.empty(Bw, N, L - 1, dtype=torch.int64, device="cuda"))
        return {"to_session": t1 - t0, "to_training": tick() - t1}

    # the cross-entropy step first and alone: interleaved with the others it would re-bind too
    forms = {"scst": scst_whole, "phases": scst_phases, "rebind": rebind}
    got = {k: [] for k in list(forms) + ["ce"]}
    for r in range(a.warm + a.steps):
        v = ce_step()
        if r >= a.warm:
            got["ce"].append(v)
    for r in range(a.warm + a.steps):
        order = list(forms.items())
        order = order[r % len(order):] + order[:r % len(order)]
        for k, fn in order:
            v = fn()
            if r >= a.warm:
                got[k].append(v)

    def ms(k, f):
        v = [1e3 * x[f] for x in got[k]]
        return f"{statistics.median(v):8.2f} ({min(v):8.2f}) ms"

    lines = [f"one step of bench.py's caption workload (B = {Bw}, bf16, FusedAdam, train mode, randomly initialised model: no sample ends "
             f"early), host wall ms with a synchronize, median (min) of {a.steps} rounds (the self-critical forms interleaved) after {a.warm} warm-up",
             f"  cross-entropy step (Lt = {Lt})                     {ms('ce', 'step')}",
             f"  self-critical step (n = {N}, greedy, L = {L})        {ms('scst', 'step')}   scst.SelfCritical.loss + backward + optimizer",
             f"  the same by hand, a synchronize between phases    {ms('phases', 'step')}",
             f"    sampling session ({Bw * N} rows, {L - 1} positions)       {ms('phases', 'sampling')}   includes its re-binding and prefill",
             f"    greedy session ({Bw} rows)                        {ms('phases', 'greedy')}   same binding, its own prefill",
             f"    two rewards launches + targets                  {ms('phases', 'rewards_targets')}",
             f"    forward + backward + optimizer ([{Bw}, {N}, {L - 1}])     {ms('phases', 'fwd_bwd_opt')}   includes its re-binding",
             f"  re-binding alone: to the session's shape          {ms('rebind', 'to_session')}",
             f"                    to the training forward's shape {ms('rebind', 'to_training')}"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--steps", type=int, default=12, help="timed rounds of the whole-step table")
    ap.add_argument("--corpus-images", type=int, default=110000)
    ap.add_argument("--step", action="store_true", help="also time a whole self-critical step beside the cross-entropy step")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scst_bench needs the GPU: nothing is measured without one")
    big, table_lines = table_rows(a)
    lines = kernel_rows(a, big) + [""] + table_lines
    del big
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
