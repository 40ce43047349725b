#!/usr/bin/env python3
"""Throughput of the gated feed-forward (T5 v1.1 / Flan-T5) on one MI355X.

1. The gate kernels (klab_geglu_fwd / klab_geglu_bwd) against the same arithmetic written as torch eager ops, at the
   t5-v1_1-small / -large training shapes: median of 50 timed launches after 10 warm-up launches (HIP events), with the achieved
   HBM bandwidth from the bytes each form must move at least (forward 3, backward 5 matrices of M x F in bf16).
2. A whole training step (forward + backward + FusedAdam, bf16, dropout on, B = 64, Ls 9, Lt 64, random init) of a
   t5-v1_1-small shaped model beside the t5-small shaped one behind the same small Swin tower, batches from bench.synth_batch.

    python tools/ffn_gated_bench.py
"""
import math
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warm=10, n=50):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def gate_bench():
    from klab_multimodalmodel_amd import ops as K
    c0 = math.sqrt(2.0 / math.pi)
    for M, F in ((64 * 64, 1024), (64 * 73, 1024), (64 * 64, 2816)):
        ab = torch.randn(M, 2 * F, device="cuda").bfloat16()
        dh = torch.randn(M, F, device="cuda").bfloat16()
        h = torch.empty(M, F, device="cuda", dtype=torch.bfloat16)
        dab = torch.empty(M, 2 * F, device="cuda", dtype=torch.bfloat16)
        sd = torch.tensor([7], dtype=torch.int32, device="cuda")

        def t_fwd():
            return torch.nn.functional.dropout(torch.nn.functional.gelu(ab[:, :F], approximate="tanh") * ab[:, F:], 0.1, True)

        def t_bwd():
            a, b = ab[:, :F].float(), ab[:, F:].float()
            t = torch.tanh(c0 * (a + 0.044715 * a ** 3))
            g = dh.float()
            da = g * b * (0.5 * (1 + t) + 0.5 * a * (1 - t * t) * c0 * (1 + 3 * 0.044715 * a * a))
            return torch.cat([da, g * 0.5 * a * (1 + t)], 1).bfloat16()

        us = dict(fwd=timed(lambda: K.geglu_fwd(ab, h, 0.1, sd, 5)), bwd=timed(lambda: K.geglu_bwd(dh, ab, dab, 0.1, sd, 5)),
                  torch_fwd=timed(t_fwd), torch_bwd=timed(t_bwd))
        mb = M * F * 2 / 1e3  # kB per M x F bf16 matrix: kB / us = GB / s
        print(f"gate M={M} F={F}: fwd {us['fwd']:.1f} us ({3 * mb / us['fwd']:.0f} GB/s) torch {us['torch_fwd']:.1f} us | "
              f"bwd {us['bwd']:.1f} us ({5 * mb / us['bwd']:.0f} GB/s) torch {us['torch_bwd']:.1f} us (no mask regeneration)")


def step_bench():
    import bench
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.hf_io import KNOWN_T5
    from klab_multimodalmodel_amd.models.model import MyModel
    from klab_multimodalmodel_amd.optim import FusedAdam
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    sw = SwinConfig(image_size=224, embed_dim=64, depths=(2, 2, 6, 2), num_heads=(2, 4, 8, 16), window_size=7)
    for name in ("t5-small", "google/t5-v1_1-small"):
        m = MyModel(args, _configs=(sw, T5Config(**KNOWN_T5["t5-small"]), T5Config(**KNOWN_T5[name])), dtype="bf16").to("cuda")
        m._direct_grads = True
        m.transformer.train()
        opt = FusedAdam(m.transformer.parameters(), lr=1e-4)
        pix, src, tgt = bench.synth_batch(64, 9, 64, 224, m.main_cfg.vocab_size, "cuda")
        images, se, te = {"pixel_values": pix}, {"input_ids": src}, {"input_ids": tgt}

        def step():
            loss = m(images, se, te)
            loss.backward()
            opt.step()
            opt.zero_grad()

        print(f"step {name}: {timed(step, warm=15, n=40) / 1e3:.3f} ms (fast Adam path: {opt._fallback is None})")
        del m, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    gate_bench()
    step_bench()
