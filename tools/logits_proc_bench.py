"""Cost of MyModel.generate's logits processors at BASELINE configs[1] shapes (B=64, max_length 20, bf16): ms per batch for greedy,
beam search (num_beams 4) and sampling (num_return_sequences 1), each without processors and with no_repeat_ngram_size=3,
repetition_penalty=1.2.  Random-init weights rarely emit EOS, so every run takes its full 19 decoder steps.
--only greedy (or beam4 / sample, optionally +procs, e.g. sample+procs): one mode only (a short run for a kernel trace)."""
import argparse, os, sys, time, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--iters", type=int, default=5)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    from klab_multimodalmodel_amd.models.model import MyModel
    sw, t5 = bench.cfg2_configs()
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="t5-small", image_model_name="swinv2-C64-224-w7",
                                 image_model_train=False, transformer_model_name="t5-small")
    model = MyModel(args, _configs=(sw, t5, t5), _seed=0, dtype="bf16").to(dev)
    pix, src, _tgt = bench.synth_batch(64, 9, 64, 224, 32128, dev, seed=1)
    procs = dict(no_repeat_ngram_size=3, repetition_penalty=1.2)
    modes = {}
    for name, kw in (("greedy", {}), ("beam4", dict(num_beams=4)), ("sample", dict(do_sample=True))):
        modes[name] = kw
        modes[name + "+procs"] = dict(kw, **procs)
    for name, kw in modes.items():
        if opt.only and name != opt.only:
            continue
        for _ in range(2):
            out = model.generate(pix, src, max_length=20, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(opt.iters):
            out = model.generate(pix, src, max_length=20, **kw)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / opt.iters
        print(f"{name}: {tuple(out.shape)} in {dt * 1e3:.2f} ms/batch => {out.shape[0] / dt:.0f} captions/s", flush=True)


if __name__ == "__main__":
    main()
