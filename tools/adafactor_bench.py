#!/usr/bin/env python3
"""Time of one optimizer step() on one MI355X, in one process, at t5-small / t5-v1_1-small (and, with --large, t5-large) sizes:

  fused     optim.FusedAdafactor on the flat buffers (four launches, csrc/adafactor.hip)
  fallback  the same rule per parameter in plain torch (what optim.FusedAdafactor falls back to; the loop
            transformers.optimization.Adafactor runs).  The fp32 -> compute-dtype cast pass the next forward then needs is
            looked for as (forward after a fallback step) - (forward right after a fused step); when that difference is
            inside the forward's own spread the output says "not resolved" and counts nothing
  adam      optim.FusedAdam (one launch)

Two figures per fused step, median of --n after --warm: GPU time between two events around step() behind a long product (what
the step costs a loop whose host runs ahead), and wall time around step() with a device synchronisation on both sides (host work included: the
ownership test walks the parameter list).  The per-parameter loop is host-bound and synchronises itself: wall time only.  The
gradients of one backward stay in place for all steps.

    python tools/adafactor_bench.py [--large]
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


_busy = None


def wall(fn, warm, n, gpu=True):
    """(GPU us between events, wall us) medians.  For the GPU figure a ~10 ms product is enqueued first, so that the host has
    finished step() long before the device reaches its launches: the events then bracket kernel time alone."""
    global _busy
    if _busy is None:
        _busy = torch.randn(8192, 8192, device="cuda")
    for _ in range(warm):
        fn()
    out, dev = [], []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e6)
    for _ in range(n if gpu else 0):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.mm(_busy, _busy)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        dev.append(a.elapsed_time(b) * 1e3)
    return (statistics.median(dev) if dev else None), statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large", action="store_true")
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--n", type=int, default=30)
    a = ap.parse_args()
    import bench
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.hf_io import KNOWN_T5
    from klab_multimodalmodel_amd.models.model import MyModel
    from klab_multimodalmodel_amd.optim import FusedAdafactor, FusedAdam
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    names = ["t5-small", "google/t5-v1_1-small"] + (["t5-large"] if a.large else [])
    for name in names:
        small = "small" in name
        B = 64 if small else 8
        # the tower's last stage and the language encoder are as wide as the main T5 (8 x embed_dim = d_model)
        sw = (SwinConfig(image_size=224, embed_dim=64, depths=(2, 2, 6, 2), num_heads=(2, 4, 8, 16), window_size=7) if small else
              SwinConfig(image_size=256, embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), window_size=8))
        lang = T5Config(**KNOWN_T5["t5-small" if small else "t5-large"])
        m = MyModel(args, _configs=(sw, lang, T5Config(**KNOWN_T5[name])), dtype="bf16").to("cuda")
        m._direct_grads = True
        m.transformer.train()
        params = list(m.transformer.parameters())
        nparam = sum(p.numel() for p in params)
        pix, src, tgt = bench.synth_batch(B, 9, 64, sw.image_size, m.main_cfg.vocab_size, "cuda")
        images, se, te = {"pixel_values": pix}, {"input_ids": src}, {"input_ids": tgt}

        def fwd():
            return m(images, se, te)

        fwd().backward()
        fused = FusedAdafactor(params)
        fused_m = FusedAdafactor(params, beta1=0.9)
        fallback = FusedAdafactor([{"params": params[:1]}, {"params": params[1:]}])  # two groups: the per-parameter torch rule
        adam = FusedAdam(params, lr=1e-5)
        us = dict(fused=wall(fused.step, a.warm, a.n), fused_beta1=wall(fused_m.step, a.warm, a.n), adam=wall(adam.step, a.warm, a.n))
        assert fused._flat_live and fused_m._flat_live and adam._fallback is None, (fused._fb_reason, adam._fb_reason)
        us["fallback"] = wall(fallback.step, 1, max(3, a.n // 6), gpu=False)[1]
        assert not fallback._flat_live

        def fwd_after(opt_step):
            def f():
                opt_step()
                torch.cuda.synchronize()
                t = time.perf_counter()
                with torch.no_grad():
                    fwd()
                torch.cuda.synchronize()
                return (time.perf_counter() - t) * 1e6
            for _ in range(3):
                f()
            return statistics.median(f() for _ in range(6))

        f_cur, f_cast = fwd_after(fused.step), fwd_after(fallback.step)
        cast = f_cast - f_cur
        cast_txt = f"+ cast {cast:.1f} us" if cast > 0 else "(cast not resolved:"
        cast = max(0.0, cast)
        print(f"{name}: {len(params)} tensors, {nparam / 1e6:.1f} M parameters, bf16 copies   (GPU us / wall us)")
        for key, label, nb in (("fused", "FusedAdafactor", 26), ("fused_beta1", "FusedAdafactor beta1", 34), ("adam", "FusedAdam", 30)):
            d, w = us[key]
            print(f"  {label:22s} {d:9.1f} / {w:9.1f} us   ({nb * nparam / d / 1e6:.2f} TB/s of the {nb} B/param model)")
        print(f"  Adafactor / Adam        GPU {us['fused'][0] / us['adam'][0]:.2f}   wall {us['fused'][1] / us['adam'][1]:.2f}")
        print(f"  torch fallback          {us['fallback']:9.1f} us wall {cast_txt} (forward {f_cast:.1f} vs {f_cur:.1f} us{')' if cast == 0 else ''}) = "
              f"{us['fallback'] + cast:.1f} us   fallback / fused (wall) = {(us['fallback'] + cast) / us['fused'][1]:.1f}")
        del m, fused, fused_m, fallback, adam, params
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
