"""End-to-end parity of the native MyModel (libklab_mm.so engine) against goldens produced by the
reference itself (tests/golden/*.npz) and against the CPU oracle: loss, tower outputs, every gradient.

Stated tolerances: fp32 engine -- loss rel <= 1e-5, grad rel-L2 <= 1e-4 per tensor;
bf16 engine -- loss rel <= 2e-3, overall grad cosine >= 0.99, per-tensor cosine >= 0.97, and rel-L2 <= 2 x the oracle's
own bf16 error on the same batch (overall and per tensor).
"""
import math
import os
import types

import pytest
import torch

from tests.helpers import cosine, load_golden, rel_l2

pytestmark = pytest.mark.gpu


def build(name, dtype, train_swin):
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_golden(name)
    sw = SwinConfig.from_dict(g["meta"]["swin_config"])
    t5 = T5Config.from_dict(g["meta"]["t5_config"])
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=train_swin,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], g["sds"]["main"]), dtype=dtype)
    return m.to("cuda"), g


def run(m, g):
    inp = g["inputs"]
    images = {"pixel_values": inp["pixel_values"].cuda()}
    src = {"input_ids": inp["src_ids"].cuda(), "attention_mask": torch.ones_like(inp["src_ids"]).cuda()}
    tgt = {"input_ids": inp["tgt_ids"].cuda(), "attention_mask": torch.ones_like(inp["tgt_ids"]).cuda()}
    return m(images, src, tgt)


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b", "tiny_c", "tiny_d"])  # c, d: padded windows (HF/swinv2:645-650), d with 100-token windows
@pytest.mark.parametrize("train_swin", [False, True])
def test_fp32_engine_matches_reference(name, train_swin):
    m, g = build(name, torch.float32, train_swin)
    m.transformer.eval()  # dropout off: the reference's parity-capable mode
    loss = run(m, g)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    eng = m._engine
    B = g["inputs"]["src_ids"].shape[0]
    cat = torch.cat([g["acts"]["image_embeddings"], g["acts"]["language_embeddings"]], dim=1)
    assert rel_l2(eng.buffer("encoder_input").float().cpu().view(B, -1, cat.shape[-1]), cat) < 2e-5
    assert rel_l2(eng.buffer("encoder_out").float().cpu().view(B, -1, cat.shape[-1]), g["acts"]["encoder_out"]) < 2e-5
    assert rel_l2(eng.buffer("decoder_out").float().cpu().view(B, -1, cat.shape[-1]), g["acts"]["decoder_out"]) < 2e-5
    assert abs(loss.item() - g["loss"]) <= 1e-5 * abs(g["loss"])
    loss.backward()
    assert int(eng.err_view.item()) == 0
    worst = ("", 0.0)
    for mname, tree in (("main", m.transformer), ("swin", m.image_model)):
        for k, ref in g["grads"][mname].items():
            p = tree.get_parameter(k)
            if mname == "swin" and not train_swin:
                assert p.grad is None
                continue
            assert p.grad is not None, k
            if float(ref.abs().max()) == 0.0:
                assert float(p.grad.abs().max()) < 1e-10, k
                continue
            e = rel_l2(p.grad.cpu(), ref)
            if e > worst[1]:
                worst = (k, e)
            assert e < 1e-4, (mname, k, e)
    for p in m.language_model.parameters():
        assert p.grad is None
    print(name, train_swin, "loss", loss.item(), "worst grad", worst)


def _oracle_bf16_cast_error(g):
    """The oracle's OWN bf16 error on this batch (SURVEY §8c yardstick): the same CPU restatement with every weight, input and
    activation in bf16, against the reference goldens.  Returns (loss rel error, {tensor name: rel-L2}, overall rel-L2)."""
    from oracle import swin_t5_oracle as O
    dt = torch.bfloat16
    sds = {m: {k: (v.to(dt) if v.is_floating_point() else v) for k, v in g["sds"][m].items()} for m in g["sds"]}
    main = {k: v.clone().requires_grad_(True) for k, v in sds["main"].items()}
    swin = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sds["swin"].items()}
    inp = g["inputs"]
    loss = O.mymodel_forward(swin, sds["lang"], main, g["swin_cfg"], g["t5_cfg"], g["t5_cfg"], inp["pixel_values"].to(dt), inp["src_ids"],
                             inp["tgt_ids"], training=False, image_model_train=True)
    loss.backward()
    per, a, b = {}, [], []
    for mname, src in (("main", main), ("swin", swin)):
        for k, ref in g["grads"][mname].items():
            if src[k].grad is None:
                continue
            got = src[k].grad.float()
            per[(mname, k)] = rel_l2(got, ref)
            a.append(got.flatten())
            b.append(ref.flatten())
    return abs(float(loss.detach()) - g["loss"]) / abs(g["loss"]), per, rel_l2(torch.cat(a), torch.cat(b))


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b", "tiny_c", "tiny_d"])
def test_bf16_engine_within_stated_tolerance(name):
    """SURVEY §8(c), bf16 kernels: loss rel <= 2e-3, gradient cosine >= 0.99 AND rel-L2 <= 2 x the oracle's own bf16 error on
    the same batch -- overall and per tensor (the per-tensor bound gets the overall oracle error as a floor: a tensor the bf16
    oracle happens to hit exactly does not set a zero bar)."""
    m, g = build(name, torch.bfloat16, True)
    m.transformer.eval()
    loss = run(m, g)
    assert abs(loss.item() - g["loss"]) <= 2e-3 * abs(g["loss"])
    loss.backward()
    _e_loss, e_per, e_all = _oracle_bf16_cast_error(g)
    a, b, viol = [], [], []
    worst = (1.0, "")
    for mname, tree in (("main", m.transformer), ("swin", m.image_model)):
        for k, ref in g["grads"][mname].items():
            got = tree.get_parameter(k).grad.cpu()
            if float(ref.norm()) > 1e-6 * ref.numel() ** 0.5:
                c = cosine(got, ref)
                worst = min(worst, (c, k))
                bound = 2 * max(e_per.get((mname, k), 0.0), e_all)
                if c <= 0.97 or rel_l2(got, ref) > bound:
                    viol.append((mname, k, "cosine", round(c, 4), "rel-L2", round(rel_l2(got, ref), 4), "bound", round(bound, 4)))
            a.append(got.flatten())
            b.append(ref.flatten())
    c = cosine(torch.cat(a), torch.cat(b))
    r = rel_l2(torch.cat(a), torch.cat(b))
    print(name, "bf16 loss", loss.item(), "ref", g["loss"], "grad cosine", c, "rel-L2", r, "oracle's own bf16 rel-L2", e_all,
          "worst per-tensor cosine", worst)
    assert not viol, viol
    assert c > 0.99, c
    assert r <= 2 * e_all, (r, e_all)


def test_eval_loss_is_repeatable_and_no_grad_works():
    m, g = build("tiny_a", torch.float32, False)
    m.transformer.eval()
    with torch.no_grad():
        l1 = run(m, g)
        l2 = run(m, g)
    assert not l1.requires_grad
    assert l1.item() == l2.item()


def test_train_mode_dropout_statistics():
    # train mode: losses differ step to step (different masks), stay near the eval loss, backward runs
    m, g = build("tiny_b", torch.float32, False)
    m.transformer.train()
    ls = []
    for _ in range(6):
        loss = run(m, g)
        loss.backward()
        ls.append(loss.item())
        for p in m.transformer.parameters():
            assert torch.isfinite(p.grad).all()
            p.grad = None
    assert len(set(ls)) > 1
    assert abs(sum(ls) / len(ls) - g["loss"]) < 0.5


def test_width_mismatch_raises_like_the_reference():
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    with pytest.raises(RuntimeError, match="Sizes of tensors must match"):
        MyModel(args, _configs=(SwinConfig(embed_dim=96), T5Config(), T5Config()))  # Swin-Tiny 768 vs t5-small 512


def _oracle_from_model(m):
    from oracle import swin_t5_oracle as O
    sc = O.SwinCfg(**{k: getattr(m.swin_cfg, k) for k in O.SwinCfg.__dataclass_fields__})
    def t5(c):
        return O.T5Cfg(**{k: getattr(c, k) for k in O.T5Cfg.__dataclass_fields__ if hasattr(c, k)})
    sds = []
    for tree in (m.image_model, m.language_model, m.transformer):
        sds.append({k: v.detach().cpu().clone() for k, v in tree.state_dict().items()})
    return O, sc, t5(m.lang_cfg), t5(m.main_cfg), sds


@pytest.mark.parametrize("dtype,loss_tol,cos_min", [(torch.float32, 2e-5, 0.99999), (torch.bfloat16, 2e-3, 0.99)])
def test_full_size_architecture_matches_oracle(dtype, loss_tol, cos_min):
    """BASELINE configs[0]/[1] architecture (Swin-V2 C=64 (2,2,6,2) 224 w7 + T5-small, V=32128) at B=2:
    exercises n=49 windows, head dim 32, the 128x128 GEMM tiles and the 32128-wide LM head."""
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    sw = SwinConfig(image_size=224, embed_dim=64, depths=(2, 2, 6, 2), num_heads=(2, 4, 8, 16), window_size=7)
    t5 = T5Config()
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _seed=3, dtype=dtype)
    O, sc, lc, mc, (ssd, lsd, msd) = _oracle_from_model(m)
    m = m.to("cuda")
    m.transformer.eval()
    g = torch.Generator().manual_seed(1234)
    B, Ls, Lt = 2, 9, 64
    pix = torch.randn(B, 3, 224, 224, generator=g)
    src = torch.randint(2, 32000, (B, Ls), generator=g)
    tgt = torch.randint(2, 32000, (B, Lt), generator=g)
    src[:, -1] = 1
    tgt[:, -1] = 1
    tgt[1, -16:] = 0  # pad tail: pads are scored
    loss = m({"pixel_values": pix.cuda()}, {"input_ids": src.cuda()}, {"input_ids": tgt.cuda()})
    loss.backward()
    msd = {k: v.requires_grad_(True) for k, v in msd.items()}
    torch.set_num_threads(8)
    ref = O.mymodel_forward(ssd, lsd, msd, sc, lc, mc, pix, src, tgt, training=False)
    ref.backward()
    assert abs(loss.item() - float(ref)) <= loss_tol * abs(float(ref)), (loss.item(), float(ref))
    a, b = [], []
    for k, p in m.transformer.named_parameters():
        a.append(p.grad.cpu().flatten())
        b.append(msd[k].grad.flatten())
    c = cosine(torch.cat(a), torch.cat(b))
    print("full-size", dtype, "loss", loss.item(), float(ref), "grad cosine", c, "rel-L2", rel_l2(torch.cat(a), torch.cat(b)))
    assert c > cos_min


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _drop_engines():
    """every model / engine of the caller is gone and the device is idle (klab DDP-wrapped models sit in a reference cycle
    with their wrapper, so only the cyclic collector frees them)"""
    import gc
    gc.collect()
    torch.cuda.synchronize()


def _train_steps(wrap, accumulate=1, steps=3, fused_adam=False, overlap=False, in_backward=False):
    """the reference's loop body (ref/train.py:58-71) on a tiny config; returns losses and final weights."""
    import torch.distributed as dist
    m, g = build("tiny_b", torch.float32, True)
    m.transformer.eval()  # deterministic (no dropout) so that the three gradient paths can be compared exactly
    if wrap == "torch":
        model = torch.nn.parallel.DistributedDataParallel(m, device_ids=[0])
        core = model.module
    elif wrap == "klab":
        from klab_multimodalmodel_amd.ddp import DistributedDataParallel
        model = DistributedDataParallel(m, device_ids=[0], overlap_optimizer=overlap)
        core = model.module
    else:
        model = core = m
    if fused_adam:
        from klab_multimodalmodel_amd.optim import FusedAdam
        opt = FusedAdam(core.transformer.parameters(), lr=1e-3, step_in_backward=in_backward)
    else:
        opt = torch.optim.Adam(core.transformer.parameters(), lr=1e-3)
    losses = []
    for i in range(steps * accumulate):
        loss = run(model, g) if wrap else run(m, g)
        losses.append(loss.item())
        (loss / accumulate).backward()
        if (i + 1) % accumulate == 0:
            if overlap and not fused_adam:
                model.join()  # a consumer other than FusedAdam has to join the pending all-reduces itself
            opt.step()
            opt.zero_grad()
    if in_backward:  # every step but the first updated segment 0 underneath the encoder's backward
        assert opt._fallback is None and opt.in_backward_updates == steps - 1, (opt._fb_reason, opt.in_backward_updates)
    w = {k: v.detach().clone() for k, v in core.transformer.state_dict().items()}
    sg = core.image_model.get_parameter("layernorm.weight").grad
    sg = None if sg is None else sg.detach().clone()
    torch.cuda.synchronize()
    del model, core, m, opt, loss  # the engine (its streams, events) goes before the caller tears the process group down
    _drop_engines()
    return losses, w, sg


def test_reference_training_loop_under_stock_ddp_and_klab_ddp():
    """`DDP(model)`, Adam over transformer.parameters(), accumulation, zero_grad -- ref/train.py:26-28,58-71.
    Stock torch DDP (autograd-hook path), klab DDP (direct flat-gradient path) and no wrapper must agree."""
    import os
    import torch.distributed as dist
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        for acc in (1, 2):
            l0, w0, s0 = _train_steps(None, acc)
            l1, w1, s1 = _train_steps("torch", acc)
            l2, w2, s2 = _train_steps("klab", acc)
            l3, w3, _s3 = _train_steps("klab", acc, fused_adam=True)  # klab DDP + klab FusedAdam (what bench.py runs at N > 1)
            os.environ["KLAB_DDP_FORCE_COLLECTIVE"] = "1"  # same, with the RCCL all-reduces really issued on the comm stream
            try:
                l4, w4, _s4 = _train_steps("klab", acc, fused_adam=True)
                # overlap_optimizer: backward leaves the last all-reduces unjoined, FusedAdam updates segment by segment
                l5, w5, _s5 = _train_steps("klab", acc, fused_adam=True, overlap=True)
                l6, w6, _s6 = _train_steps("klab", acc, fused_adam=False, overlap=True)  # torch Adam behind an explicit ddp.join()
                if acc == 1:  # FusedAdam(step_in_backward=True): segment 0 updated behind ITS all-reduce, underneath the encoder backward
                    for ov in (False, True):
                        l7, w7, _s7 = _train_steps("klab", acc, fused_adam=True, overlap=ov, in_backward=True)
                        assert max(abs(x - y) for x, y in zip(l0, l7)) < 2e-4, (ov, l0, l7)
                        for k in w0:
                            assert rel_l2(w7[k].cpu(), w0[k].cpu()) < 2e-3, (ov, k)
            finally:
                del os.environ["KLAB_DDP_FORCE_COLLECTIVE"]
            assert max(abs(x - y) for x, y in zip(l0, l4)) < 2e-4, (acc, l0, l4)
            assert max(abs(x - y) for x, y in zip(l0, l5)) < 2e-4, (acc, l0, l5)
            assert max(abs(x - y) for x, y in zip(l0, l6)) < 2e-4, (acc, l0, l6)
            for k in w0:
                assert rel_l2(w4[k].cpu(), w0[k].cpu()) < 2e-3, k
                assert rel_l2(w5[k].cpu(), w0[k].cpu()) < 2e-3, k
            assert max(abs(x - y) for x, y in zip(l0, l3)) < 2e-4, (acc, l0, l3)
            for k in w0:
                assert rel_l2(w3[k].cpu(), w0[k].cpu()) < 2e-3, k
            assert l0[0] > l0[-1]  # it learns the batch
            for a, b in ((l0, l1), (l0, l2)):
                assert max(abs(x - y) for x, y in zip(a, b)) < 2e-4, (acc, a, b)
            for k in w0:
                assert rel_l2(w1[k].cpu(), w0[k].cpu()) < 2e-3, k  # Adam normalises: last-bit gradient differences (atomics) grow
                assert rel_l2(w2[k].cpu(), w0[k].cpu()) < 2e-3, k
            # Swin gradients are computed and accumulate forever (never zeroed by the optimizer: SURVEY §0.4)
            assert s0 is not None and s1 is not None and s2 is not None
            assert rel_l2(s1.cpu(), s0.cpu()) < 1e-3 and rel_l2(s2.cpu(), s0.cpu()) < 1e-3
    finally:
        _drop_engines()  # no engine, comm stream or in-flight collective is left when the communicator goes
        dist.destroy_process_group()


def test_generate_greedy_matches_oracle_argmax():
    m, g = build("tiny_b", torch.float32, False)
    inp = g["inputs"]
    out = m({"pixel_values": inp["pixel_values"].cuda()}, {"input_ids": inp["src_ids"].cuda()}, return_loss=False)
    assert out.shape[0] == inp["src_ids"].shape[0] and out.shape[1] <= 20 and int(out[0, 0]) == 0
    # first generated token == argmax of the oracle's logits at decoder position 0
    from oracle import swin_t5_oracle as O
    sds = g["sds"]
    tgt = torch.zeros(inp["src_ids"].shape[0], 1, dtype=torch.long)
    _, parts = O.mymodel_forward(sds["swin"], sds["lang"], sds["main"], g["swin_cfg"], g["t5_cfg"], g["t5_cfg"], inp["pixel_values"],
                                 inp["src_ids"], tgt, return_parts=True)
    assert torch.equal(out[:, 1].cpu(), parts["logits"][:, 0].argmax(-1))


def test_generate_kv_cache_matches_prefix_recompute():
    """decoding over the K/V cache (the decoding session: one new position per row, the session's per-layer
    q|k|v cache, cross K/V from the prefill) yields token for token what re-running the decoder over the whole prefix yields --
    fp32: identical ids and logits to 1e-5; bf16: logits within bf16 round-off (an argmax may flip on a near-tie of
    random-weight logits, so ids are compared in fp32 only).  The step-level half drives a pick session by hand and overwrites
    the tokens it chose with a fixed prefix before every step."""
    for dtype in (torch.float32, torch.bfloat16):
        m, g = build("tiny_b", dtype, False)
        inp = g["inputs"]
        pix, src = inp["pixel_values"].cuda(), inp["src_ids"].cuda()
        a = m.generate(pix, src, max_length=12, kv_cache=True)
        b = m.generate(pix, src, max_length=12, kv_cache=False)
        assert a.shape == b.shape and int(a[0, 0]) == 0
        if dtype == torch.float32:
            assert torch.equal(a, b), (a, b)
        # step-level check on a fixed prefix: logits of position t from the cache path vs the full-prefix path
        B = src.shape[0]
        steps = 11
        cfg = m.main_cfg
        tgt = torch.randint(2, g["t5_cfg"].vocab_size, (B, steps), generator=torch.Generator().manual_seed(1)).cuda()
        eng = m._engine_for(pix, src, tgt)
        m.transformer.eval()
        with torch.no_grad():
            eng.forward(pix, src, tgt, training=0, seed=m._seed_base, want_grad=False)
            full = eng.buffer("logits").view(B, steps, -1).float().clone()  # teacher-forced logits of every position
            # replay the same prefix through the cache: decoder input at t is tgt[:, t-1] (shift right)
            eng.forward(pix, src, torch.zeros_like(tgt), training=0, seed=m._seed_base, want_grad=False)  # prefill with another target
            gen = eng.gen_cfg("pick", 1, steps + 1, cfg.eos_token_id, cfg.pad_token_id)
            ws = torch.empty(eng.gen_workspace_bytes(gen), dtype=torch.uint8, device="cuda")
            eng.gen_begin(gen, ws)
            for t in range(1, steps):
                eng.gen_buffer(ws, "tokens").copy_(tgt[:, t - 1])
                eng.gen_step(t, ws)
                step = eng.gen_buffer(ws, "logits").float()
                assert step.shape == full[:, t].shape
                err = rel_l2(step.cpu(), full[:, t].cpu())
                assert err < (1e-5 if dtype == torch.float32 else 2e-2), (dtype, t, err)


def test_hipgraph_replay_matches_eager():
    """eager first step, captured second step, replayed afterwards: identical loss and gradients to the eager engine,
    with fresh input tensors every step (inputs are staged, so replay must not depend on their addresses)."""
    res = {}
    for graph in (False, True):
        m, g = build("tiny_b", torch.float32, True)
        m.use_graph = graph
        m.transformer.eval()
        out = []
        for step in range(4):
            inp = {k: v.clone() for k, v in g["inputs"].items()}
            if step == 3:
                inp["tgt_ids"] = inp["tgt_ids"].flip(1).contiguous()  # different data through the same graph
            loss = m({"pixel_values": inp["pixel_values"].cuda()}, {"input_ids": inp["src_ids"].cuda()}, {"input_ids": inp["tgt_ids"].cuda()})
            loss.backward()
            gq = m.transformer.get_parameter("decoder.block.0.layer.1.EncDecAttention.q.weight").grad.detach().clone()
            gs = m.image_model.get_parameter("layernorm.weight").grad.detach().clone()
            out.append((loss.item(), gq, gs))
            m.zero_grad(set_to_none=True)
        res[graph] = out
        del m, loss  # (klab_engine_destroy drains in-flight replays itself: test_engine_teardown_with_work_in_flight)
    for (l0, q0, s0), (l1, q1, s1) in zip(res[False], res[True]):
        assert abs(l0 - l1) <= 1e-6 * abs(l0)
        assert rel_l2(q1.cpu(), q0.cpu()) < 1e-5 and rel_l2(s1.cpu(), s0.cpu()) < 1e-4
    assert abs(res[True][0][0] - res[True][1][0]) < 1e-6 and abs(res[True][3][0] - res[True][0][0]) > 1e-3
    # train mode under replay: the device-side RNG counter still advances => losses differ step to step
    m, g = build("tiny_b", torch.float32, False)
    m.use_graph = True
    m.transformer.train()
    ls = []
    for _ in range(5):
        loss = run(m, g)
        loss.backward()
        ls.append(loss.item())
        m.zero_grad(set_to_none=True)
    assert len(set(ls)) == 5


def test_engine_teardown_with_work_in_flight():
    """Regression for the round-1 GPU-suite crash: an engine dropped or re-bound while its last backward --
    eager kernels on the side stream, or replayed hipGraphs on the caller's stream -- is still executing.  klab_engine_destroy /
    klab_engine_bind now drain the device before they release graph executables, events, streams and (the caller) the
    workspace; the next engine's results must be unaffected."""
    ref = None
    for graph in (False, True, True):
        m, g = build("tiny_b", torch.float32, True)
        m.use_graph = graph
        m.transformer.eval()
        for _ in range(3):  # eager, captured, replayed
            loss = run(m, g)
            loss.backward()
            m.zero_grad(set_to_none=True)
        loss = run(m, g)
        loss.backward()  # left in flight: no synchronisation before the model goes
        lv = loss  # (device scalar: reading it below is the first sync)
        gq = m.transformer.get_parameter("decoder.block.0.layer.1.EncDecAttention.q.weight").grad
        # re-bind to another batch shape with the previous backward still running, then drop everything
        inp = g["inputs"]
        m({"pixel_values": inp["pixel_values"][:1].cuda()}, {"input_ids": inp["src_ids"][:1].cuda()}, {"input_ids": inp["tgt_ids"][:1].cuda()})
        val = (float(lv), gq.detach().clone())
        del m, loss, lv, gq
        if ref is None:
            ref = val
        else:
            assert abs(val[0] - ref[0]) <= 1e-6 * abs(ref[0])
    torch.cuda.synchronize()


def test_frozen_tower_caches_follow_weight_updates():
    """the engine keeps bf16 copies / CPB tables of the frozen towers across steps; an in-place weight change
    (load_state_dict, manual edit) must invalidate them through the tensors' version counters."""
    m, g = build("tiny_a", torch.float32, False)
    m.transformer.eval()
    with torch.no_grad():
        l1 = run(m, g).item()
        l2 = run(m, g).item()  # cached path
        assert l1 == l2
        m.language_model.get_parameter("encoder.block.0.layer.0.SelfAttention.q.weight").mul_(1.5)
        l3 = run(m, g).item()
        assert abs(l3 - l1) > 1e-6
        sd = m.image_model.state_dict()
        sd["encoder.layers.0.blocks.0.attention.self.continuous_position_bias_mlp.2.weight"] = \
            sd["encoder.layers.0.blocks.0.attention.self.continuous_position_bias_mlp.2.weight"] * -2.0
        m.image_model.load_state_dict(sd)
        l4 = run(m, g).item()
        assert abs(l4 - l3) > 1e-7
        assert run(m, g).item() == l4


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_fused_adam_matches_torch_adam(dtype, wd):
    """optim.FusedAdam (one kernel over the flat buffers, bf16 copies refreshed, forward's cast skipped) follows
    torch.optim.Adam (ref/train.py:28) step for step: same parameters after 4 steps in eval mode (no dropout noise)."""
    from klab_multimodalmodel_amd.optim import FusedAdam
    ms, opts = [], []
    for fused in (False, True):
        m, g = build("tiny_a", dtype, False)
        m._direct_grads = True
        m.transformer.eval()
        ps = list(m.transformer.parameters())
        opts.append(FusedAdam(ps, lr=3e-3, weight_decay=wd) if fused else torch.optim.Adam(ps, lr=3e-3, weight_decay=wd))
        ms.append(m)
    losses = [[], []]
    for step in range(4):
        for k in (0, 1):
            loss = run(ms[k], g)
            loss.backward()
            opts[k].step()
            opts[k].zero_grad()
            losses[k].append(float(loss))
    assert opts[1]._fallback is None, opts[1]._fb_reason          # the one-kernel path really ran
    assert ms[1]._trainable_current()                              # ... and the next forward would skip its cast
    tol = 2e-5 if dtype == torch.float32 else 2e-3                 # bf16: both sides see bf16-rounded gradients of slightly different weights
    for a, b in zip(losses[0], losses[1]):
        assert abs(a - b) <= tol * abs(a) + 1e-6
    worst = 0.0
    for (n0, p0), (_n1, p1) in zip(ms[0].transformer.named_parameters(), ms[1].transformer.named_parameters()):
        worst = max(worst, rel_l2(p1.detach().cpu(), p0.detach().cpu()))
    assert worst < (1e-5 if dtype == torch.float32 else 2e-2), worst  # bf16: atomics-order noise in tiny gradients, amplified by Adam
    # the skipped cast did not leave stale copies behind: an explicit in-place write to a weight is noticed (version counter)
    with torch.no_grad():
        next(ms[1].transformer.parameters()).mul_(1.0)
    assert not ms[1]._trainable_current()
    # state_dict is torch.optim.Adam compatible
    sd = opts[1].state_dict()
    ref_sd = opts[0].state_dict()
    assert set(sd["state"].keys()) == set(ref_sd["state"].keys())
    k0 = next(iter(sd["state"]))
    assert set(sd["state"][k0].keys()) >= {"step", "exp_avg", "exp_avg_sq"}
    assert rel_l2(sd["state"][k0]["exp_avg"].cpu(), ref_sd["state"][k0]["exp_avg"].cpu()) < (1e-4 if dtype == torch.float32 else 2e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_adam_step_in_backward(dtype):
    """optim.FusedAdam(step_in_backward=True): the update of backward segment 0 runs on a side stream underneath the encoder's
    backward, segment 1 at step().  Same arithmetic as the one-kernel step: same weights and Adam state after 5 steps, with
    dropout ON (the mask stream is a function of the step count only), and a forward that nobody followed with step() joins."""
    from klab_multimodalmodel_amd.optim import FusedAdam
    ms, opts = [], []
    for inb in (False, True):
        m, g = build("tiny_b", dtype, False)
        m._direct_grads = True
        m.transformer.train()
        opts.append(FusedAdam(m.transformer.parameters(), lr=2e-3, weight_decay=0.01, step_in_backward=inb))
        ms.append(m)
    for step in range(5):
        ls = []
        for k in (0, 1):
            loss = run(ms[k], g)
            loss.backward()
            opts[k].step()
            opts[k].zero_grad()
            ls.append(float(loss))
        assert abs(ls[0] - ls[1]) <= (2e-5 if dtype == torch.float32 else 3e-3) * abs(ls[0]) + 1e-6, (step, ls)
    assert opts[1]._fallback is None and opts[1].in_backward_updates == 4 and opts[0].in_backward_updates == 0
    assert ms[1]._trainable_current()
    worst = 0.0
    for (n0, p0), (_n1, p1) in zip(ms[0].transformer.named_parameters(), ms[1].transformer.named_parameters()):
        worst = max(worst, rel_l2(p1.detach().cpu(), p0.detach().cpu()))
    assert worst < (1e-5 if dtype == torch.float32 else 2e-2), worst
    assert rel_l2(opts[1]._m.cpu(), opts[0]._m.cpu()) < (1e-4 if dtype == torch.float32 else 3e-2)
    assert rel_l2(opts[1]._v.cpu(), opts[0]._v.cpu()) < (1e-4 if dtype == torch.float32 else 3e-2)
    # a backward whose step() never comes: the next forward still orders itself behind the in-flight segment-0 update
    run(ms[1], g).backward()
    assert ms[1]._pending_opt_stream is not None
    with torch.no_grad():
        run(ms[1], g)
    assert ms[1]._pending_opt_stream is None
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_checkpoint_resume_with_fused_adam(tmp_path):
    """MyModel.save()/load() (ref/models/model.py:30-42 schema) + optimizer.state_dict() give a true resume:
    2 steps, save, fresh model + optimizer, load, 2 more steps == 4 uninterrupted steps (fp32, eval mode)."""
    from klab_multimodalmodel_amd.optim import FusedAdam

    def make():
        m, g = build("tiny_a", torch.float32, False)
        m.args.result_dir = str(tmp_path)
        m._direct_grads = True
        m.transformer.eval()
        return m, g, FusedAdam(m.transformer.parameters(), lr=2e-3)

    def steps(m, g, opt, n):
        out = []
        for _ in range(n):
            loss = run(m, g)
            loss.backward()
            opt.step()
            opt.zero_grad()
            out.append(float(loss))
        return out

    m0, g, o0 = make()
    ref = steps(m0, g, o0, 4)
    m1, g, o1 = make()
    first = steps(m1, g, o1, 2)
    m1.save("ck.pth")
    torch.save(o1.state_dict(), os.path.join(str(tmp_path), "opt.pth"))
    m2, g, o2 = make()
    m2.load("ck.pth")
    run(m2, g)  # binds the engine (the optimizer state is laid out like its flat gradient buffer)
    o2.load_state_dict(torch.load(os.path.join(str(tmp_path), "opt.pth")))
    rest = steps(m2, g, o2, 2)
    assert o2._fallback is None, o2._fb_reason
    for a, b in zip(ref, first + rest):
        assert abs(a - b) <= 2e-5 * abs(a) + 1e-6, (ref, first + rest)


@pytest.mark.gpu
def test_dropout_stream_survives_rebinds():
    """The reference loop pads every batch to its longest row (ref/train.py:56-57), so (Ls, Lt) -- and with it the engine's
    binding -- changes almost every step.  The dropout RNG (base seed + forward counter) belongs to the model, not to the
    binding: alternating two shapes must keep counting (different masks every step), and a restored (base, counter) must
    continue the same stream across the next shape change."""
    def make():
        m, g = build("tiny_a", torch.float32, False)
        m._seed_base = 4321
        m.transformer.train()
        return m, g

    def fwd(m, g, short):
        inp = g["inputs"]
        tgt = inp["tgt_ids"][:, :5] if short else inp["tgt_ids"]
        src = inp["src_ids"][:, :4] if short else inp["src_ids"]
        with torch.no_grad():
            return float(m({"pixel_values": inp["pixel_values"].cuda()}, {"input_ids": src.contiguous().cuda()}, {"input_ids": tgt.contiguous().cuda()}))

    m0, g = make()
    seq = [fwd(m0, g, k % 2 == 1) for k in range(6)]  # shapes A B A B A B: five rebinds
    assert m0._engine.get_rng() == (4321, 6)
    assert len({round(x, 7) for x in seq[0::2]}) == 3 and len({round(x, 7) for x in seq[1::2]}) == 3, seq  # same input, new masks
    m1, g = make()
    for k in range(2):
        fwd(m1, g, k % 2 == 1)
    base, ctr = m1._engine.get_rng()
    assert (base, ctr) == (4321, 2)
    m2, g = make()
    m2._seed_base = base
    m2._pending_rng = (base, ctr)  # what load_checkpoint does before the first forward
    rest = [fwd(m2, g, k % 2 == 1) for k in range(2, 6)]
    for a, b in zip(seq[2:], rest):
        assert abs(a - b) <= 1e-6 * abs(a), (seq, rest)


def test_resume_continues_the_dropout_stream(tmp_path):
    """true resume with dropout ON: the engine's device-side RNG (base seed + forward counter) and the model's seed base are
    part of the checkpoint, so 2 steps + save + load into a fresh model + 2 steps reproduce 4 uninterrupted train-mode steps
    (without them the resumed run would replay the masks of steps 1-2)."""
    from klab_multimodalmodel_amd.checkpoint import AsyncCheckpointer, load_checkpoint
    from klab_multimodalmodel_amd.optim import FusedAdam

    def make(seed_base):
        m, g = build("tiny_a", torch.float32, False)
        m._seed_base = seed_base
        m._direct_grads = True
        m.transformer.train()
        return m, g, FusedAdam(m.transformer.parameters(), lr=2e-3)

    def steps(m, g, opt, n):
        out = []
        for _ in range(n):
            loss = run(m, g)
            loss.backward()
            opt.step()
            opt.zero_grad()
            out.append(float(loss))
        return out

    m0, g, o0 = make(1234)
    ref = steps(m0, g, o0, 4)
    assert len(set(ref)) == 4
    m1, g, o1 = make(1234)
    first = steps(m1, g, o1, 2)
    assert m1._engine.get_rng() == (1234, 2)
    ck = AsyncCheckpointer(str(tmp_path))
    ck.save(m1, o1, None, step=2, name="d.pth")
    ck.wait()
    for early in (False, True):  # load after one binding forward / before any forward (state applied at bind)
        m2, g, o2 = make(999)  # a different base: the checkpoint's must win
        if not early:
            run(m2, g)
            assert load_checkpoint(os.path.join(str(tmp_path), "d.pth"), m2, o2) == 2
            rest = steps(m2, g, o2, 2)
            assert o2._fallback is None, o2._fb_reason
            for a, b in zip(ref, first + rest):
                assert abs(a - b) <= 2e-5 * abs(a) + 1e-6, (ref, first + rest)
        else:
            ckd = torch.load(os.path.join(str(tmp_path), "d.pth"), weights_only=False)
            assert ckd["engine_rng"]["seed_base"] == 1234 and [int(x) for x in ckd["engine_rng"]["state"][1:]] == [1234, 2]
            m2.transformer.load_state_dict(ckd["transformer"])
            m2._seed_base = 1234
            m2._pending_rng = (1234, 2)
            l3 = float(run(m2, g))  # step 3's forward: same weights (before its update), same masks
            assert abs(l3 - ref[2]) <= 2e-5 * abs(ref[2]) + 1e-6


@pytest.mark.gpu
def test_full_batch_properties_at_bench_size():
    """BASELINE configs[1] at its full size (B=64, Ls=9, Lt=64, bf16) has no oracle run that finishes in seconds, so the hot path
    is checked through size-independent properties: (1) the mean-token loss and the gradients of the whole batch equal the
    average over its two halves (same token counts; eval mode, so no dropout); (2) backward is linear in d(loss);
    (3) a repeated forward reproduces the loss bit for bit."""
    import bench
    from klab_multimodalmodel_amd.models.model import MyModel
    sw, t5 = bench.cfg2_configs()
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _seed=0, dtype="bf16").to("cuda")
    m._direct_grads = True
    m.transformer.eval()
    B = 64
    pix, src, tgt = bench.synth_batch(B, 9, 64, 224, 32128, "cuda", seed=77)

    def run_part(sl, scale=1.0):
        for p in m.transformer.parameters():
            p.grad = None
        loss = m({"pixel_values": pix[sl]}, {"input_ids": src[sl]}, {"input_ids": tgt[sl]})
        (loss * scale).backward()
        return float(loss), torch.cat([p.grad.flatten() for p in m.transformer.parameters() if p.grad is not None]).double().clone()

    l_full, g_full = run_part(slice(0, B))
    l_again, _ = run_part(slice(0, B))
    assert l_full == l_again
    l_a, g_a = run_part(slice(0, B // 2))
    l_b, g_b = run_part(slice(B // 2, B))
    assert abs(l_full - 0.5 * (l_a + l_b)) <= 1e-3 * abs(l_full), (l_full, l_a, l_b)
    g_avg = 0.5 * (g_a + g_b)
    cos = float(torch.dot(g_full, g_avg) / (g_full.norm() * g_avg.norm()))
    assert cos > 0.999, cos
    assert abs(float(g_full.norm() / g_avg.norm()) - 1.0) < 2e-2
    _, g_2 = run_part(slice(0, B), scale=2.0)
    cos2 = float(torch.dot(g_full, g_2) / (g_full.norm() * g_2.norm()))
    assert cos2 > 0.9995 and abs(float(g_2.norm() / g_full.norm()) - 2.0) < 2e-2, (cos2, float(g_2.norm() / g_full.norm()))


@pytest.mark.gpu
def test_async_sharded_checkpoint_resume(tmp_path):
    """AsyncCheckpointer (snapshot on a side stream, background write, Adam moments sharded over 2 ranks) +
    load_checkpoint: 2 steps, save, fresh model, load, 2 more == 4 uninterrupted steps; training continues while the file is written."""
    from klab_multimodalmodel_amd.checkpoint import AsyncCheckpointer, load_checkpoint
    from klab_multimodalmodel_amd.optim import FusedAdam

    def make():
        m, g = build("tiny_a", torch.float32, False)
        m.args.result_dir = str(tmp_path)
        m._direct_grads = True
        m.transformer.eval()
        return m, g, FusedAdam(m.transformer.parameters(), lr=2e-3)

    def steps(m, g, opt, n):
        out = []
        for _ in range(n):
            loss = run(m, g)
            loss.backward()
            opt.step()
            opt.zero_grad()
            out.append(float(loss))
        return out

    m0, g, o0 = make()
    ref = steps(m0, g, o0, 4)
    m1, g, o1 = make()
    first = steps(m1, g, o1, 2)
    ck = AsyncCheckpointer(str(tmp_path))
    ck.save(m1, o1, None, step=2, name="s.pth", rank=0, world=2)
    steps(m1, g, o1, 1)  # training goes on; the snapshot must not see this step
    ck.save(m1, o1, None, step=3, name="later.pth", rank=0, world=1)
    ck.wait()
    # rank 1 of the first save (same replica state in real DDP; here re-created by replaying)
    m1b, g, o1b = make()
    steps(m1b, g, o1b, 2)
    ck.save(m1b, o1b, None, step=2, name="s.pth", rank=1, world=2)
    ck.wait()
    assert os.path.exists(os.path.join(str(tmp_path), "s.pth.opt0of2")) and os.path.exists(os.path.join(str(tmp_path), "s.pth.opt1of2"))
    m2, g, o2 = make()
    run(m2, g)  # binds the engine: the flat buffers exist
    assert load_checkpoint(os.path.join(str(tmp_path), "s.pth"), m2, o2) == 2
    rest = steps(m2, g, o2, 2)
    assert o2._fallback is None, o2._fb_reason
    for a, b in zip(ref, first + rest):
        assert abs(a - b) <= 2e-5 * abs(a) + 1e-6, (ref, first + rest)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,loss_tol,cos_min", [(torch.float32, 3e-5, 0.9999), (torch.bfloat16, 3e-3, 0.99)])
def test_config3_architecture_with_trainable_swin_matches_oracle(dtype, loss_tol, cos_min):
    """BASELINE configs[2]/[3] architecture as SURVEY §8(d) resolves it -- Swin-V2 C=96 heads (3,6,12,24) 224 w7, UNFROZEN, +
    T5-base (d=768, 12 heads, ff 3072), V=32128 -- at B=1 with the Swin depth cut to (2,2,2,2) and 3+3 T5 layers so that the
    CPU oracle finishes in seconds: exercises widths 96/192/384/768 (3-k-tile GEMMs, 24-lane LayerNorm rows, 768-wide
    RMS-norm), 12-head attention and the Swin backward kernels at n=49."""
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    sw = SwinConfig(image_size=224, embed_dim=96, depths=(2, 2, 2, 2), num_heads=(3, 6, 12, 24), window_size=7)
    t5 = T5Config(d_model=768, d_ff=3072, num_heads=12, num_layers=3, num_decoder_layers=3)
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=True,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _seed=5, dtype=dtype)
    O, sc, lc, mc, (ssd, lsd, msd) = _oracle_from_model(m)
    m = m.to("cuda")
    m.transformer.eval()
    g = torch.Generator().manual_seed(77)
    B, Ls, Lt = 1, 9, 32
    pix = torch.randn(B, 3, 224, 224, generator=g)
    src = torch.randint(2, 32000, (B, Ls), generator=g)
    tgt = torch.randint(2, 32000, (B, Lt), generator=g)
    tgt[0, -5:] = 0
    loss = m({"pixel_values": pix.cuda()}, {"input_ids": src.cuda()}, {"input_ids": tgt.cuda()})
    loss.backward()
    msd = {k: v.requires_grad_(True) for k, v in msd.items()}
    ssd = {k: (v.requires_grad_(True) if v.is_floating_point() else v) for k, v in ssd.items()}
    torch.set_num_threads(8)
    ref = O.mymodel_forward(ssd, lsd, msd, sc, lc, mc, pix, src, tgt, training=False, image_model_train=True)
    ref.backward()
    assert abs(loss.item() - float(ref)) <= loss_tol * abs(float(ref)), (loss.item(), float(ref))
    for tree, sd, name in ((m.transformer, msd, "t5"), (m.image_model, ssd, "swin")):
        a, b = [], []
        for k, p in tree.named_parameters():
            if p.grad is None or sd[k].grad is None:
                continue
            a.append(p.grad.cpu().flatten())
            b.append(sd[k].grad.flatten())
        c = cosine(torch.cat(a), torch.cat(b))
        print("cfg3-arch", dtype, name, "grad cosine", c, "rel-L2", rel_l2(torch.cat(a), torch.cat(b)))
        assert c > cos_min, (name, c)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,loss_tol,cos_min", [(torch.float32, 3e-5, 0.9999), (torch.bfloat16, 3e-3, 0.99)])
def test_spanmask_workload_matches_oracle(dtype, loss_tol, cos_min):
    """BASELINE configs[3] (RedCaps span-mask pre-training, ref/modules/loader.py:56-72): the configs[2] architecture at the
    span-mask shapes Ls=32, Lt=16 with `<extra_id_k>` sentinel ids (32099 - k) in source and target, ragged rows padded with
    id 0 (pads are scored).  Depth cut (Swin (2,2,2,2), 3+3 T5 layers) so that the CPU oracle finishes in seconds;
    B=4 covers one short row.  Ids near the top of the vocabulary exercise the last LM-head / embedding tiles."""
    import bench
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    sw = SwinConfig(image_size=224, embed_dim=96, depths=(2, 2, 2, 2), num_heads=(3, 6, 12, 24), window_size=7)
    t5 = T5Config(d_model=768, d_ff=3072, num_heads=12, num_layers=3, num_decoder_layers=3)
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=True,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _seed=11, dtype=dtype)
    O, sc, lc, mc, (ssd, lsd, msd) = _oracle_from_model(m)
    m = m.to("cuda")
    m.transformer.eval()
    B, Ls, Lt = 4, 32, 16
    pix, src, tgt = bench.synth_spanmask_batch(B, Ls, Lt, 224, 32128, "cpu", seed=5)
    assert int(src.max()) == 32099 and int(tgt[0, 0]) == 32099 and int((tgt == 0).sum()) > 0 and int((src[3] == 0).sum()) > 0
    for b in range(B):  # the sentinel grammar of the loader: <extra_id_0> w.. <extra_id_1> ... <extra_id_4> </s>
        sent = [int(x) for x in tgt[b] if int(x) >= 32000]
        assert sent == [32099 - k for k in range(len(sent))] and len(sent) >= 4
    loss = m({"pixel_values": pix.cuda()}, {"input_ids": src.cuda()}, {"input_ids": tgt.cuda()})
    loss.backward()
    assert int(m._engine.err_view.item()) == 0
    msd = {k: v.requires_grad_(True) for k, v in msd.items()}
    ssd = {k: (v.requires_grad_(True) if v.is_floating_point() else v) for k, v in ssd.items()}
    torch.set_num_threads(8)
    ref = O.mymodel_forward(ssd, lsd, msd, sc, lc, mc, pix, src, tgt, training=False, image_model_train=True)
    ref.backward()
    assert abs(loss.item() - float(ref)) <= loss_tol * abs(float(ref)), (loss.item(), float(ref))
    for tree, sd, name in ((m.transformer, msd, "t5"), (m.image_model, ssd, "swin")):
        a, b = [], []
        for k, p in tree.named_parameters():
            if p.grad is None or sd[k].grad is None:
                continue
            a.append(p.grad.cpu().flatten())
            b.append(sd[k].grad.flatten())
        c = cosine(torch.cat(a), torch.cat(b))
        print("spanmask", dtype, name, "grad cosine", c, "rel-L2", rel_l2(torch.cat(a), torch.cat(b)))
        assert c > cos_min, (name, c)
    # the sentinel rows of the tied embedding really received gradient (decoder input gather + LM head)
    gs = m.transformer.get_parameter("shared.weight").grad[32095:32100].abs().sum(1).cpu()
    assert bool((gs > 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["cfg3", "spanmask"])
def test_full_depth_unfrozen_swin_properties_at_bench_size(workload):
    """BASELINE configs[2] / configs[3] per-GPU slices at FULL size (Swin-V2 C=96 (2,2,18,2) unfrozen + 12+12-layer T5-base,
    B=32, bf16), where no oracle run finishes in seconds: size-independent properties of the hot path --
    loss / T5 + Swin gradients of the whole batch = average over its two halves; backward linear in d(loss); a repeated
    forward is bit-identical; no out-of-range id flagged."""
    import bench
    from klab_multimodalmodel_amd.models.model import MyModel
    wl = bench.WORKLOADS[workload]
    sw, t5 = bench.workload_configs(workload)
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=True,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _seed=0, dtype="bf16").to("cuda")
    m._direct_grads = True
    m.transformer.eval()
    B, Ls, Lt = wl["B"], wl["Ls"], wl["Lt"]
    synth = bench.synth_spanmask_batch if wl["span"] else bench.synth_batch
    pix, src, tgt = synth(B, Ls, Lt, 224, 32128, "cuda", seed=77)
    trees = (m.transformer, m.image_model)

    def run_part(sl, scale=1.0):
        for t in trees:
            for p in t.parameters():
                p.grad = None
        loss = m({"pixel_values": pix[sl]}, {"input_ids": src[sl]}, {"input_ids": tgt[sl]})
        (loss * scale).backward()
        return float(loss), [torch.cat([p.grad.flatten() for p in t.parameters() if p.grad is not None]).double().clone() for t in trees]

    l_full, g_full = run_part(slice(0, B))
    l_again, _ = run_part(slice(0, B))
    assert l_full == l_again and int(m._engine.err_view.item()) == 0
    l_a, g_a = run_part(slice(0, B // 2))
    l_b, g_b = run_part(slice(B // 2, B))
    assert abs(l_full - 0.5 * (l_a + l_b)) <= 1e-3 * abs(l_full), (l_full, l_a, l_b)
    for gf, ga, gb, name in zip(g_full, g_a, g_b, ("t5", "swin")):
        g_avg = 0.5 * (ga + gb)
        cos = float(torch.dot(gf, g_avg) / (gf.norm() * g_avg.norm()))
        assert cos > 0.995, (name, cos)
        assert abs(float(gf.norm() / g_avg.norm()) - 1.0) < 3e-2, name
    _, g_2 = run_part(slice(0, B), scale=2.0)
    for gf, g2, name in zip(g_full, g_2, ("t5", "swin")):
        cos2 = float(torch.dot(gf, g2) / (gf.norm() * g2.norm()))
        assert cos2 > 0.999 and abs(float(g2.norm() / gf.norm()) - 2.0) < 3e-2, (name, cos2)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,loss_tol,cos_min", [(torch.float32, 3e-5, 0.9999), (torch.bfloat16, 3e-3, 0.99)])
def test_large_window_swin_matches_oracle(dtype, loss_tol, cos_min):
    """BASELINE configs[4] style tower at a size the CPU oracle finishes in seconds: window 24 with pretrained_window_sizes
    (12,12,12,6) on a 192 px image -> stage 0: four SHIFTED windows of 576 tokens, stage 1: one window of 576 (R <= window: no
    shift, HF/swinv2:615-618), stage 2: 144 tokens, stage 3: 36 -- the tiled large-window attention forward / backward, the
    bias-table CPB path and the one-tile kernels in one model; unfrozen Swin, every T5 and Swin gradient against the oracle."""
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    sw = SwinConfig(image_size=192, embed_dim=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), window_size=24,
                    pretrained_window_sizes=(12, 12, 12, 6))
    t5 = T5Config(vocab_size=512, d_model=256, d_kv=32, num_heads=4, d_ff=512, num_layers=2)
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=True,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _seed=21, dtype=dtype)
    O, sc, lc, mc, (ssd, lsd, msd) = _oracle_from_model(m)
    m = m.to("cuda")
    m.transformer.eval()
    g = torch.Generator().manual_seed(3)
    B, Ls, Lt = 2, 5, 7
    pix = torch.randn(B, 3, 192, 192, generator=g)
    src = torch.randint(2, 500, (B, Ls), generator=g)
    tgt = torch.randint(2, 500, (B, Lt), generator=g)
    loss = m({"pixel_values": pix.cuda()}, {"input_ids": src.cuda()}, {"input_ids": tgt.cuda()})
    loss.backward()
    msd = {k: v.requires_grad_(True) for k, v in msd.items()}
    ssd = {k: (v.requires_grad_(True) if v.is_floating_point() else v) for k, v in ssd.items()}
    torch.set_num_threads(8)
    ref = O.mymodel_forward(ssd, lsd, msd, sc, lc, mc, pix, src, tgt, training=False, image_model_train=True)
    ref.backward()
    assert abs(loss.item() - float(ref)) <= loss_tol * abs(float(ref)), (loss.item(), float(ref))
    for tree, sd, name in ((m.transformer, msd, "t5"), (m.image_model, ssd, "swin")):
        a, b = [], []
        for k, p in tree.named_parameters():
            if p.grad is None or sd[k].grad is None:
                continue
            if dtype == torch.float32 and float(sd[k].grad.norm()) > 1e-7:
                assert rel_l2(p.grad.cpu(), sd[k].grad) < 2e-3, (name, k, rel_l2(p.grad.cpu(), sd[k].grad))
            a.append(p.grad.cpu().flatten())
            b.append(sd[k].grad.flatten())
        c = cosine(torch.cat(a), torch.cat(b))
        print("large-window", dtype, name, "grad cosine", c, "rel-L2", rel_l2(torch.cat(a), torch.cat(b)))
        assert c > cos_min, (name, c)


@pytest.mark.gpu
@pytest.mark.parametrize("window,dtype,train_swin", [(8, torch.float32, True), (8, torch.bfloat16, True), (8, torch.bfloat16, False),
                                                     (16, torch.float32, True), (16, torch.bfloat16, True), (16, torch.bfloat16, False)])
def test_reference_default_window_geometry_matches_oracle(window, dtype, train_swin):
    """The reference's LITERAL default tower geometry (ref/modules/config.py:6-11: `swinv2-base-patch4-window8-256`; the
    `window16-256` checkpoint the CLI also accepts): 256 px, patch 4 -> 64x64 tokens.  Window 8: n = 64 tokens = exactly the
    one-tile limit of the small-window kernels, shifted by 4 in stages 0-2, R = w = 8 in stage 3.  Window 16: n = 256 (the
    streaming kernels) in stages 0-1, R = w in stage 2, window clamped to 8 in stage 3 (HF/swinv2:615-618).  Depth and width cut
    (C = 32, head dim 32 as in every named checkpoint) so that the CPU oracle finishes in seconds; frozen (the fused frozen-tower
    kernels at n = 64) and unfrozen towers; loss, the tower's output rows and every gradient against the oracle."""
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    sw = SwinConfig(image_size=256, embed_dim=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), window_size=window)
    t5 = T5Config(vocab_size=512, d_model=256, d_kv=32, num_heads=4, d_ff=512, num_layers=2)
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=train_swin,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _seed=31 + window, dtype=dtype)
    O, sc, lc, mc, (ssd, lsd, msd) = _oracle_from_model(m)
    m = m.to("cuda")
    m.transformer.eval()
    g = torch.Generator().manual_seed(5)
    B, Ls, Lt = 2, 5, 9
    pix = torch.randn(B, 3, 256, 256, generator=g)
    src = torch.randint(2, 500, (B, Ls), generator=g)
    tgt = torch.randint(2, 500, (B, Lt), generator=g)
    loss = m({"pixel_values": pix.cuda()}, {"input_ids": src.cuda()}, {"input_ids": tgt.cuda()})
    loss.backward()
    msd = {k: v.requires_grad_(True) for k, v in msd.items()}
    if train_swin:
        ssd = {k: (v.requires_grad_(True) if v.is_floating_point() else v) for k, v in ssd.items()}
    torch.set_num_threads(8)
    ref, parts = O.mymodel_forward(ssd, lsd, msd, sc, lc, mc, pix, src, tgt, training=False, image_model_train=train_swin, return_parts=True)
    ref.backward()
    f32 = dtype == torch.float32
    assert abs(loss.item() - float(ref)) <= (3e-5 if f32 else 3e-3) * abs(float(ref)), (loss.item(), float(ref))
    cat = torch.cat([parts["image_embeddings"], parts["language_embeddings"]], dim=1).detach()
    got = m._engine.buffer("encoder_input").float().cpu().view(B, -1, cat.shape[-1])
    assert rel_l2(got, cat) < (2e-5 if f32 else 2e-2), rel_l2(got, cat)
    trees = [(m.transformer, msd, "t5")] + ([(m.image_model, ssd, "swin")] if train_swin else [])
    for tree, sd, name in trees:
        a, b = [], []
        for k, p in tree.named_parameters():
            if p.grad is None or sd[k].grad is None:
                continue
            if f32 and float(sd[k].grad.norm()) > 1e-7:
                assert rel_l2(p.grad.cpu(), sd[k].grad) < 2e-3, (name, k, rel_l2(p.grad.cpu(), sd[k].grad))
            a.append(p.grad.cpu().flatten())
            b.append(sd[k].grad.flatten())
        c = cosine(torch.cat(a), torch.cat(b))
        print("ref-default geometry w", window, dtype, "train_swin", train_swin, name, "grad cosine", c, "rel-L2", rel_l2(torch.cat(a), torch.cat(b)))
        assert c > (0.9999 if f32 else 0.99), (name, c)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_configs4_architecture_runs_at_full_width(mode):
    """BASELINE configs[4] as SURVEY §8(d) resolves it -- Swin-V2 C=128 (2,2,18,2) heads (4,8,16,32) 384 px window 24,
    pretrained_window_sizes (12,12,12,6), unfrozen + T5-large widths -- binds and steps (no KLAB_ERR_UNSUPPORTED); T5 depth cut to
    2+2 layers to keep the test short.  Properties: finite loss and gradients, repeated forward bit-identical, backward linear."""
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    sw = SwinConfig(image_size=384, embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), window_size=24,
                    pretrained_window_sizes=(12, 12, 12, 6))
    t5 = T5Config(d_model=1024, d_ff=4096, num_heads=16, num_layers=2, num_decoder_layers=2)
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=True,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _seed=2, dtype=mode).to("cuda")  # fp8: BASELINE configs[4]'s own mode
    m._direct_grads = True
    m.transformer.eval()
    import bench
    pix, src, tgt = bench.synth_batch(2, 9, 64, 384, 32128, "cuda", seed=9)

    def run_once(scale):
        for t in (m.transformer, m.image_model):
            for p in t.parameters():
                p.grad = None
        loss = m({"pixel_values": pix}, {"input_ids": src}, {"input_ids": tgt})
        (loss * scale).backward()
        gs = torch.cat([p.grad.flatten() for p in m.image_model.parameters() if p.grad is not None]).double()
        gt = torch.cat([p.grad.flatten() for p in m.transformer.parameters() if p.grad is not None]).double()
        return float(loss), gs.clone(), gt.clone()

    l1, gs1, gt1 = run_once(1.0)
    l2, gs2, gt2 = run_once(2.0)
    assert l1 == l2 and math.isfinite(l1) and int(m._engine.err_view.item()) == 0
    assert bool(torch.isfinite(gs1).all()) and bool(torch.isfinite(gt1).all()) and float(gs1.norm()) > 0
    for a, b in ((gs1, gs2), (gt1, gt2)):
        assert float(torch.dot(a, b) / (a.norm() * b.norm())) > 0.999 and abs(float(b.norm() / a.norm()) - 2.0) < 3e-2


class _Fp8Linear(torch.autograd.Function):
    """F.linear with both operands cast to per-row-scaled e4m3 in the forward pass and a full-precision backward: the
    'oracle cast' of SURVEY §8(c)'s tolerance rule for the fp8 mode (what an ideal fp8 forward costs in accuracy)."""

    @staticmethod
    def forward(ctx, x, w, b):
        from tests.helpers import fp8_rows
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        qx, sx = fp8_rows(x.reshape(-1, x.shape[-1]))
        qw, sw = fp8_rows(w)
        y = ((qx * sx) @ (qw * sw).t()).view(*x.shape[:-1], w.shape[0]).to(x.dtype)
        return y + b if b is not None else y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = g @ w
        gw = g.reshape(-1, g.shape[-1]).t() @ x.reshape(-1, x.shape[-1])
        return gx, gw, (g.reshape(-1, g.shape[-1]).sum(0) if ctx.has_b else None)


@pytest.mark.gpu
def test_fp8_forward_mode_within_twice_the_oracle_cast_error():
    """dtype="fp8" (BASELINE configs[4]'s "fp8 MFMA path"): forward Linear GEMMs on e4m3 operands with per-row scales, bf16
    everywhere else.  Stated tolerance: error against the fp32 oracle <= 2 x the error of the oracle itself with
    its Linear operands cast to e4m3 (+ the bf16 mode's own allowance), gradient cosine >= 0.98."""
    import torch.nn.functional as F
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    sw = SwinConfig(image_size=224, embed_dim=64, depths=(2, 2, 2, 2), num_heads=(2, 4, 8, 16), window_size=7)
    t5 = T5Config(d_model=512, d_ff=2048, num_heads=8, num_layers=2, num_decoder_layers=2)
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=True,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _seed=4, dtype="fp8")
    O, sc, lc, mc, (ssd, lsd, msd) = _oracle_from_model(m)
    m = m.to("cuda")
    m.transformer.eval()
    assert m._engine._cfg.dtype == 2
    g = torch.Generator().manual_seed(8)
    B, Ls, Lt = 2, 9, 32
    pix = torch.randn(B, 3, 224, 224, generator=g)
    src = torch.randint(2, 32000, (B, Ls), generator=g)
    tgt = torch.randint(2, 32000, (B, Lt), generator=g)
    loss = m({"pixel_values": pix.cuda()}, {"input_ids": src.cuda()}, {"input_ids": tgt.cuda()})
    loss.backward()
    msd = {k: v.requires_grad_(True) for k, v in msd.items()}
    torch.set_num_threads(8)
    ref = O.mymodel_forward(ssd, lsd, msd, sc, lc, mc, pix, src, tgt, training=False)
    ref.backward()
    real_linear = F.linear
    try:  # the oracle's own fp8 cast: every F.linear of the path with e4m3 operands
        O.F.linear = lambda x, w, b=None: _Fp8Linear.apply(x, w, b)
        with torch.no_grad():
            cast = O.mymodel_forward(ssd, lsd, {k: v.detach() for k, v in msd.items()}, sc, lc, mc, pix, src, tgt, training=False)
    finally:
        O.F.linear = real_linear
    e_cast = abs(float(cast) - float(ref)) / abs(float(ref))
    e_ours = abs(loss.item() - float(ref)) / abs(float(ref))
    print("fp8 mode: loss", loss.item(), "oracle", float(ref), "oracle-with-e4m3-cast", float(cast), "rel err ours", e_ours, "cast", e_cast)
    assert e_ours <= 2 * e_cast + 2e-3, (e_ours, e_cast)
    a, b = [], []
    for k, p in m.transformer.named_parameters():
        a.append(p.grad.cpu().flatten())
        b.append(msd[k].grad.flatten())
    c = cosine(torch.cat(a), torch.cat(b))
    print("fp8 mode: T5 grad cosine", c)
    assert c > 0.98, c


@pytest.mark.gpu
def test_fp8_mode_on_the_configs4_architecture_within_twice_the_oracle_cast_error():
    """BASELINE configs[4] in ITS OWN mode: dtype="fp8" on the 384 px / window 24 tower (576- and 144-token windows, shifted and
    unshifted, pretrained_window_sizes (12,12,12,6), C = 128 with heads (4,8,16,32)) + T5-large WIDTHS (d_model 1024, d_ff 4096,
    16 heads of 64, Le = 144 + 9 = 153: the streaming T5 attention, K = 1024 / 4096 products), depth cut to (2,2,2,2) / 2+2 layers
    so that the CPU oracle finishes in seconds.  Stated tolerance: |loss - fp32 oracle| <= 2 x the error of the
    oracle itself with every Linear's operands cast to per-row e4m3 (+ the bf16 allowance 2e-3); gradient cosine >= 0.98 (T5)
    and >= 0.95 (Swin, whose forward Linears are fp8 too)."""
    import torch.nn.functional as F
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    sw = SwinConfig(image_size=384, embed_dim=128, depths=(2, 2, 2, 2), num_heads=(4, 8, 16, 32), window_size=24,
                    pretrained_window_sizes=(12, 12, 12, 6))
    t5 = T5Config(d_model=1024, d_kv=64, d_ff=4096, num_heads=16, num_layers=2, num_decoder_layers=2)
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=True,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _seed=12, dtype="fp8")
    O, sc, lc, mc, (ssd, lsd, msd) = _oracle_from_model(m)
    m = m.to("cuda")
    m.transformer.eval()
    assert m._engine._cfg.dtype == 2
    g = torch.Generator().manual_seed(18)
    B, Ls, Lt = 1, 9, 16
    pix = torch.randn(B, 3, 384, 384, generator=g)
    src = torch.randint(2, 32000, (B, Ls), generator=g)
    tgt = torch.randint(2, 32000, (B, Lt), generator=g)
    loss = m({"pixel_values": pix.cuda()}, {"input_ids": src.cuda()}, {"input_ids": tgt.cuda()})
    loss.backward()
    assert int(m._engine.err_view.item()) == 0
    msd = {k: v.requires_grad_(True) for k, v in msd.items()}
    ssd = {k: (v.requires_grad_(True) if v.is_floating_point() else v) for k, v in ssd.items()}
    torch.set_num_threads(8)
    ref = O.mymodel_forward(ssd, lsd, msd, sc, lc, mc, pix, src, tgt, training=False, image_model_train=True)
    ref.backward()
    real_linear = F.linear
    try:  # the oracle's own fp8 cast: every F.linear of the path with e4m3 operands
        O.F.linear = lambda x, w, b=None: _Fp8Linear.apply(x, w, b)
        with torch.no_grad():
            cast = O.mymodel_forward({k: v.detach() for k, v in ssd.items()}, lsd, {k: v.detach() for k, v in msd.items()}, sc, lc, mc, pix, src,
                                     tgt, training=False, image_model_train=True)
    finally:
        O.F.linear = real_linear
    e_cast = abs(float(cast) - float(ref)) / abs(float(ref))
    e_ours = abs(loss.item() - float(ref)) / abs(float(ref))
    print("fp8 on configs[4] widths: loss", loss.item(), "oracle", float(ref), "oracle-with-e4m3-cast", float(cast), "rel err ours", e_ours,
          "cast", e_cast)
    cos = {}
    for tree, sd, name in ((m.transformer, msd, "t5"), (m.image_model, ssd, "swin")):
        a, b = [], []
        for k, p in tree.named_parameters():
            if p.grad is None or sd[k].grad is None:
                continue
            a.append(p.grad.cpu().flatten())
            b.append(sd[k].grad.flatten())
        cos[name] = cosine(torch.cat(a), torch.cat(b))
        print("fp8 on configs[4] widths:", name, "grad cosine", cos[name], "rel-L2", rel_l2(torch.cat(a), torch.cat(b)))
    assert e_ours <= 2 * e_cast + 2e-3, (e_ours, e_cast)
    assert cos["t5"] > 0.98 and cos["swin"] > 0.95, cos
