"""Candidate scoring at BASELINE configs[1] shapes (B=64, bf16, candidates of L=19 tokens, N in {1, 8} per image): ms per
MyModel.score call -- one prefill at B rows, then a force session of B*N rows on the shared cross K/V -- and, in the same run, ms
of the only alternative there was before it: one teacher-forced evaluation forward over the images replicated N times (Swin and
both encoders paid N times over; the log-probabilities would still have to be gathered from its logits).
The candidates are random ids without EOS, so every row takes all its L - 1 decoder steps (the upper end of the cost).
--only score-n8 (or score-n1 / forward-n1 / forward-n8): one leg only (a short run for a kernel trace)."""
import argparse, os, sys, time, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench

B, L = 64, 19


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--iters", type=int, default=10)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    from klab_multimodalmodel_amd.models.model import MyModel
    sw, t5 = bench.cfg2_configs()
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="t5-small", image_model_name="swinv2-C64-224-w7",
                                 image_model_train=False, transformer_model_name="t5-small")
    model = MyModel(args, _configs=(sw, t5, t5), _seed=0, dtype="bf16").to(dev)
    pix, src, _tgt = bench.synth_batch(B, 9, 64, 224, 32128, dev, seed=1)
    gen = torch.Generator().manual_seed(2)
    for n in (1, 8):
        cand = torch.randint(2, 32100, (B, n, L), generator=gen).to(dev)
        if not opt.only or opt.only == f"score-n{n}":
            dt = timed(lambda: model.score(pix, src, cand), opt.iters)
            print(f"score-n{n}: {B}x{n} candidates of {L} tokens in {dt * 1e3:.2f} ms/call => {B * n / dt:.0f} candidates/s", flush=True)
        if not opt.only or opt.only == f"forward-n{n}":
            pr, sr, tgt = pix.repeat_interleave(n, 0).contiguous(), src.repeat_interleave(n, 0).contiguous(), cand.view(B * n, L).contiguous()
            model.transformer.eval()
            eng = model._engine_for(pr, sr, tgt)
            with torch.no_grad():
                dt = timed(lambda: eng.forward(pr, sr, tgt, training=0, seed=0, want_grad=False), opt.iters)
            print(f"forward-n{n}: evaluation forward at {B * n} rows in {dt * 1e3:.2f} ms/call", flush=True)


if __name__ == "__main__":
    main()
