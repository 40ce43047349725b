"""Beam-search generation (MyModel.generate(num_beams > 1)) against HF's `_beam_search` as the reference runs it
(tests/golden/beam.npz from make_beam_goldens.py), and its three kernels (csrc/beam.hip, klab_t5_beam_decode_attn) against
torch restatements."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

from tests.beam_ref import update_reference
from tests.helpers import GOLD, load_golden

pytestmark = pytest.mark.gpu


def _lib():
    from klab_multimodalmodel_amd import _lib as L
    return L, L.load()


def _build(name, dtype, eos_row=None, train_swin=False):
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_golden(name)
    sw = SwinConfig.from_dict(g["meta"]["swin_config"])
    t5 = T5Config.from_dict(g["meta"]["t5_config"])
    main = dict(g["sds"]["main"])
    if eos_row is not None:
        main["shared.weight"] = main["shared.weight"].clone()
        main["shared.weight"][1] = torch.from_numpy(eos_row)
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=train_swin,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], main), dtype=dtype)
    return m.to("cuda"), g


# ---- klab_beam_topk ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [384, 32128])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_beam_topk_kernel_matches_torch(V, k, dtype):
    L, lib = _lib()
    B = 5
    g = torch.Generator().manual_seed(V + 7 * k)
    # background logits below 0, and per row 2k planted winners on a 0.25 grid (exact in bf16): no near-ties among the candidates
    x = torch.rand(B * k, V, generator=g) * -12.0
    for r in range(B * k):
        pos = torch.randperm(V, generator=g)[:2 * k]
        x[r, pos] = 2.0 + 0.25 * torch.randperm(2 * k, generator=g).float() + 0.0625 * (r % 4)
    x = x.to(dtype).cuda()
    for first in (True, False):
        rs = torch.zeros(B, k)
        if first:
            rs[:, 1:] = -1e9
        else:
            rs = -torch.rand(B, k, generator=g) * 3.0 - torch.arange(k).float() * 0.37
        rs = rs.cuda().contiguous()
        rsc = torch.empty(B * k, 2 * k, device="cuda")
        ri = torch.empty(B * k, 2 * k, dtype=torch.int32, device="cuda")
        osc = torch.empty(B, 2 * k, device="cuda")
        oi = torch.empty(B, 2 * k, dtype=torch.int32, device="cuda")
        L.check(lib.klab_beam_topk(L.dtype_code(dtype), x.data_ptr(), V, 1, rs.data_ptr(), B, k, V, rsc.data_ptr(), ri.data_ptr(),
                                   osc.data_ptr(), oi.data_ptr(), L.stream_ptr()), "klab_beam_topk")
        ref = (torch.log_softmax(x.float(), -1) + rs.view(-1, 1)).view(B, k * V)
        rv, rix = torch.topk(ref, 2 * k, dim=-1)
        torch.cuda.synchronize()
        assert torch.equal(oi.long(), rix), (first, oi, rix)
        assert torch.allclose(osc, rv, atol=1e-5, rtol=0), (osc - rv).abs().max()


# ---- klab_t5_beam_decode_attn ----------------------------------------------------------------------------------------------
def _attn_formula(q, k, v, bias, dt):
    """T5's decode attention on the host in dtype dt: q [R, H, dk], k / v [R, Lk, H, dk], bias [H, Lk] or None -> [R, H*dk];
    unscaled q.k + the bias row, softmax, .v (HF/t5:196-197)"""
    q, k, v = q.cpu().to(dt), k.cpu().to(dt), v.cpu().to(dt)
    s = torch.einsum("rhc,rjhc->rhj", q, k)
    if bias is not None:
        s = s + bias.cpu().to(dt)[None]
    return torch.einsum("rhj,rjhc->rhc", torch.softmax(s, -1), v).reshape(q.shape[0], -1)


# Largest |kernel - fp64 formula| of the former plain one-row entry point (removed since: the same kernel with kv_group 1 and no
# table) on the two fp32 inputs of the test below, measured on an MI355X at the commit before its removal: 9.110e-07 (slot-table
# case, Lk 6 with bias) and 1.0756e-06 (kv_group case, Lk 11 without); torch's own fp32 evaluation of the formula is at 1.030e-06 and
# 1.039e-06.  The test allows 4x the kernel's figure: it uses the fast exponential and a lane-split reduction order.  In bf16 the
# bound is 2x the error of torch's own bf16 evaluation of the formula against fp64, computed in the test (measured: torch 1.825e-02
# and 2.458e-02, the kernel 6.97e-03 and 7.28e-03).
DECODE_ATTN_FP32_ERR = {"slot": 9.110426046898823e-07, "group": 1.0755508413895498e-06}


def _check_against_formula(case, out, q, k, v, bias, dtype):
    ref = _attn_formula(q, k, v, bias, torch.float64)
    err = float((out.cpu().double() - ref).abs().max())
    if dtype == torch.float32:
        bound = 4 * DECODE_ATTN_FP32_ERR[case]
    else:
        bound = 2 * float((_attn_formula(q, k, v, bias, dtype).double() - ref).abs().max())
    print(case, dtype, "max |kernel - fp64|", err, "bound", bound)
    assert err <= bound, (case, dtype, err, bound)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_beam_decode_attn_slot_table_matches_gather(dtype):
    """the key-slot table against the same kernel on a gathered copy of the cache (kv_group 1, no table), kv_group against a
    repeated copy of the keys, and both against the fp64 formula on the host"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(3)
    H, dk, B, k, Lmax, Lk, Le = 2, 32, 3, 4, 9, 6, 11
    inner = H * dk
    R = B * k
    dt = L.dtype_code(dtype)
    q = torch.randn(R, 3 * inner, generator=g).to(dtype).cuda()
    cache = torch.randn(R * Lmax, 3 * inner, generator=g).to(dtype).cuda()
    slot = torch.randint(0, R, (R, Lmax), generator=g, dtype=torch.int32).cuda()
    bias = torch.randn(H, Lmax, generator=g).cuda()
    out = torch.empty(R, inner, dtype=dtype, device="cuda")
    L.check(lib.klab_t5_beam_decode_attn(dt, q.data_ptr(), 3 * inner, cache[:, inner:].data_ptr(), cache[:, 2 * inner:].data_ptr(),
                                         Lmax * 3 * inner, 3 * inner, 1, slot.data_ptr(), Lmax, bias.data_ptr(), Lmax, out.data_ptr(), inner,
                                         R, H, Lk, dk, L.stream_ptr()), "klab_t5_beam_decode_attn")
    rows = (slot[:, :Lk].long() * Lmax + torch.arange(Lk, device="cuda")).reshape(-1)
    gath = cache[rows].contiguous()  # [R*Lk, 3*inner]
    ref = torch.empty_like(out)
    L.check(lib.klab_t5_beam_decode_attn(dt, q.data_ptr(), 3 * inner, gath[:, inner:].data_ptr(), gath[:, 2 * inner:].data_ptr(),
                                         Lk * 3 * inner, 3 * inner, 1, None, 0, bias.data_ptr(), Lmax, ref.data_ptr(), inner, R, H, Lk, dk,
                                         L.stream_ptr()), "klab_t5_beam_decode_attn")
    tol = 1e-6 if dtype == torch.float32 else 1e-2
    assert torch.allclose(out.float(), ref.float(), atol=tol, rtol=0)
    gv = gath.view(R, Lk, 3, H, dk)
    _check_against_formula("slot", out, q[:, :inner].view(R, H, dk), gv[:, :, 1], gv[:, :, 2], bias[:, :Lk], dtype)
    # kv_group: k query rows per sample share the sample's keys
    kv = torch.randn(B * Le, 2 * inner, generator=g).to(dtype).cuda()
    qc = torch.randn(R, inner, generator=g).to(dtype).cuda()
    L.check(lib.klab_t5_beam_decode_attn(dt, qc.data_ptr(), inner, kv.data_ptr(), kv[:, inner:].data_ptr(), Le * 2 * inner, 2 * inner, k,
                                         None, 0, None, 0, out.data_ptr(), inner, R, H, Le, dk, L.stream_ptr()), "klab_t5_beam_decode_attn")
    kve = kv.view(B, Le, 2 * inner).repeat_interleave(k, 0).reshape(R * Le, 2 * inner).contiguous()
    L.check(lib.klab_t5_beam_decode_attn(dt, qc.data_ptr(), inner, kve.data_ptr(), kve[:, inner:].data_ptr(), Le * 2 * inner, 2 * inner, 1,
                                         None, 0, None, 0, ref.data_ptr(), inner, R, H, Le, dk, L.stream_ptr()), "klab_t5_beam_decode_attn")
    assert torch.allclose(out.float(), ref.float(), atol=tol, rtol=0)
    kv4 = kve.view(R, Le, 2, H, dk)
    _check_against_formula("group", out, qc.view(R, H, dk), kv4[:, :, 0], kv4[:, :, 1], None, dtype)


# ---- klab_beam_update against the restatement of HF's helpers (tests/beam_ref.py: update_reference) ---------------------------------
def _state(B, k, Lm, g, c, full, unsat):
    run_seq = torch.randint(2, 50, (B, k, Lm), generator=g)
    run_seq[:, :, 0] = 0
    run_seq[:, :, c:] = 1
    fin_seq = torch.randint(2, 50, (B, k, Lm), generator=g)
    fin_seq[:, :, 0] = 0
    fin_flag = torch.rand(B, k, generator=g) < 0.5
    if full:
        fin_flag[:] = True
    fin_score = torch.where(fin_flag, -torch.rand(B, k, generator=g) * 4 - 0.5, torch.full((B, k), -1.0e9))
    return dict(run_seq=run_seq, fin_seq=fin_seq, fin_flag=fin_flag, fin_score=fin_score,
                fin_len=torch.full((B, k), c - 1, dtype=torch.int32), unsat=torch.full((B, 1), bool(unsat)))


@pytest.mark.parametrize("es", [False, True, "never"])
@pytest.mark.parametrize("lp", [1.0, 0.0, 2.0])
def test_beam_update_matches_reference_step(es, lp):
    L, lib = _lib()
    B, k, V, Lm, eos = 3, 4, 50, 8, 1
    K2 = 2 * k
    g = torch.Generator().manual_seed(5)
    scenarios = [  # (cur_len, pool full, heuristic unsatisfied, EOS candidate positions)
        (3, False, True, [0]), (3, False, True, [k + 1]), (4, True, True, [1, k]), (2, False, True, []),
        (4, True, False, [0]), (Lm - 1, False, True, []), (5, True, True, [0, 1, 2, 3])]
    for c, full, unsat, eos_at in scenarios:
        st = _state(B, k, Lm, g, c, full, unsat)
        cs = -(torch.rand(B, K2, generator=g) * 0.3 + torch.arange(K2).float() * 0.5 + 0.2)  # sorted, distinct
        beam = torch.randint(0, k, (B, K2), generator=g)
        tok = torch.stack([torch.randperm(V - 2, generator=g)[:K2] + 2 for _ in range(B)])
        tok[:, eos_at] = eos
        ci = beam * V + tok
        ref = update_reference(st, cs, ci, c, dict(k=k, V=V, Lm=Lm, eos=eos, lp=lp, es={False: 0, True: 1, "never": 2}[es]))
        dev = {n: t.cuda().contiguous() for n, t in st.items()}
        run_out = torch.zeros_like(dev["run_seq"])
        fin_out = torch.zeros_like(dev["fin_seq"])
        fin_flag = dev["fin_flag"].int().contiguous()
        unsat_d = dev["unsat"].int().view(-1).contiguous()
        run_score = torch.zeros(B, k, device="cuda")
        prev = torch.zeros(B * k, dtype=torch.int64, device="cuda")
        parent = torch.zeros(B * k, dtype=torch.int32, device="cuda")
        stop = torch.zeros(Lm, dtype=torch.int32, device="cuda")
        slot_in = torch.arange(B * k * Lm, dtype=torch.int32, device="cuda").view(B * k, Lm) % (B * k)
        slot_out = torch.full_like(slot_in, -7)
        cs_d, ci_d = cs.cuda().contiguous(), ci.int().cuda().contiguous()
        a = L.BeamUpdateArgs(B, k, V, Lm, eos, {False: 0, True: 1, "never": 2}[es], lp, cs_d.data_ptr(), ci_d.data_ptr(),
                             dev["run_seq"].data_ptr(), run_out.data_ptr(), run_score.data_ptr(), dev["fin_seq"].data_ptr(), fin_out.data_ptr(),
                             dev["fin_score"].data_ptr(), fin_flag.data_ptr(), dev["fin_len"].data_ptr(), unsat_d.data_ptr(),
                             slot_in.data_ptr(), slot_out.data_ptr(), prev.data_ptr(), parent.data_ptr(), stop.data_ptr())
        L.check(lib.klab_beam_update(C.byref(a), c, L.stream_ptr()), "klab_beam_update")
        torch.cuda.synchronize()
        what = (c, full, unsat, eos_at, es, lp)
        assert torch.equal(dev["fin_score"].cpu(), ref["fin_score"]), what
        assert torch.equal(fin_flag.cpu().bool(), ref["fin_flag"]), what
        fl = ref["fin_flag"]
        assert torch.equal(fin_out.cpu()[fl], ref["fin_seq"][fl]), what  # unfinished pool entries are placeholders
        assert torch.equal(dev["fin_len"].cpu()[fl], ref["fin_len"][fl]), what
        assert torch.equal(unsat_d.cpu().bool(), ref["unsat"].view(-1)), what
        assert int(stop[c]) == ref["word"], what
        if c + 1 >= Lm:
            continue  # every candidate hit max_length: the running beams tie at -1e9 and the search ends here
        assert torch.equal(run_out.cpu(), ref["run_seq"]), what
        assert torch.equal(run_score.cpu(), ref["run_score"]), what
        assert torch.equal(prev.cpu().view(B, k), ref["tok"]), what
        assert torch.equal(parent.cpu().view(B, k).long(), ref["par"] + torch.arange(B)[:, None] * k), what
        par = parent.cpu().long()
        so = slot_out.cpu()
        assert torch.equal(so[:, :c], slot_in.cpu()[par, :c]) and torch.equal(so[:, c], torch.arange(B * k, dtype=torch.int32)), what


# ---- MyModel.generate(num_beams > 1) --------------------------------------------------------------------------------------
def _beam_cases():
    meta = json.load(open(os.path.join(GOLD, "beam.json")))
    return meta["cases"]


def test_generate_beam_matches_reference():
    z = np.load(os.path.join(GOLD, "beam.npz"))
    cases = _beam_cases()
    assert len(cases) >= 12
    models = {}
    for cs in cases:
        key = (cs["model"], cs["variant"])
        if key not in models:
            models[key] = _build(cs["model"], "fp32", z[f"{cs['model']}.eos_row"] if cs["variant"] == "eos" else None)
        m, g = models[key]
        inp = g["inputs"]
        seq, sc = m.generate(inp["pixel_values"].cuda(), inp["src_ids"].cuda(), max_length=cs["max_length"], num_beams=cs["num_beams"],
                             length_penalty=cs["length_penalty"], early_stopping=cs["early_stopping"],
                             num_return_sequences=cs["num_return_sequences"], return_scores=True)
        want = torch.from_numpy(z[cs["id"] + ".seq"])
        assert torch.equal(seq.cpu(), want), (cs["id"], seq.cpu(), want)
        assert torch.allclose(sc.cpu(), torch.from_numpy(z[cs["id"] + ".scores"]), atol=1e-4, rtol=0), cs["id"]


def _teacher_forced_scores(m, pix, src, seq, lp, eos, pad):
    """summed token log-probabilities of a teacher-forced eval forward, / len**lp (HF's finished-hypothesis score)"""
    n = seq.shape[0]
    B = pix.shape[0]
    r = n // B
    tgt = seq[:, 1:].contiguous()
    eng = m._engine_for(pix.repeat_interleave(r, 0).contiguous(), src.repeat_interleave(r, 0).contiguous(), tgt)
    eng.forward(pix.repeat_interleave(r, 0).contiguous(), src.repeat_interleave(r, 0).contiguous(), tgt, training=0, seed=0, want_grad=False)
    logp = torch.log_softmax(eng.buffer("logits").float().view(n, tgt.shape[1], -1), -1)
    tok_lp = logp.gather(-1, tgt.unsqueeze(-1)).squeeze(-1)
    out = []
    for i in range(n):
        t = tgt[i].tolist()
        ln = t.index(eos) + 1 if eos in t else len(t)
        out.append(float(tok_lp[i, :ln].sum()) / (ln ** lp))
    return torch.tensor(out)


def _check_self_consistent(m, pix, src, k, ml, lp):
    cfg = m.main_cfg
    seq, sc = m.generate(pix, src, max_length=ml, num_beams=k, num_return_sequences=k, length_penalty=lp, return_scores=True)
    seq2, sc2 = m.generate(pix, src, max_length=ml, num_beams=k, num_return_sequences=k, length_penalty=lp, return_scores=True)
    assert torch.equal(seq, seq2) and torch.equal(sc, sc2)
    B = src.shape[0]
    assert seq.shape[0] == B * k and (seq[:, 0] == cfg.decoder_start_token_id).all()
    s = sc.view(B, k)
    assert (s[:, :-1] >= s[:, 1:]).all()
    fill = cfg.pad_token_id or cfg.eos_token_id
    for row in seq.tolist():
        if cfg.eos_token_id in row[1:]:
            e = row.index(cfg.eos_token_id, 1)
            assert all(x == fill for x in row[e + 1:])
    tf = _teacher_forced_scores(m, pix, src, seq, lp, cfg.eos_token_id, fill)
    assert torch.allclose(sc.cpu(), tf, atol=0.05 + 0.01 * tf.abs().max(), rtol=0.0), (sc.cpu(), tf)


def test_generate_beam_scores_self_consistent():
    m, g = _build("tiny_b", "bf16")
    inp = g["inputs"]
    for lp in (1.0, 2.0):
        _check_self_consistent(m, inp["pixel_values"].cuda(), inp["src_ids"].cuda(), 4, 12, lp)


def test_generate_beam_self_consistent_configs1_shapes():
    import bench
    from klab_multimodalmodel_amd.models.model import MyModel
    cfgs = bench.cfg2_configs()
    sw, t5 = cfgs[0], cfgs[1]
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _seed=0, dtype="bf16").to("cuda")
    gen = torch.Generator().manual_seed(0)
    B = 64
    pix = torch.randn(B, 3, sw.image_size, sw.image_size, generator=gen).cuda()
    src = torch.randint(2, t5.vocab_size, (B, 16), generator=gen).cuda()
    _check_self_consistent(m, pix, src, 4, 20, 1.0)


def test_generate_beam_keeps_training_binding():
    """a beam generate between two forward + backward steps changes neither their loss nor their gradients (dropout off, so the
    comparison does not depend on the dropout stream) and restores transformer.training"""
    def step(m, g):
        inp = g["inputs"]
        m.transformer.eval()
        for p in m.transformer.parameters():
            p.grad = None
        loss = m({"pixel_values": inp["pixel_values"].cuda()}, {"input_ids": inp["src_ids"].cuda()}, {"input_ids": inp["tgt_ids"].cuda()})
        loss.backward()
        torch.cuda.synchronize()
        return float(loss), m.flat_grads().clone()

    m, g = _build("tiny_b", "fp32")
    m0, _ = _build("tiny_b", "fp32")
    la, ga = step(m, g)
    lb, gb = step(m0, g)
    inp = g["inputs"]
    m.transformer.train()
    m.generate(inp["pixel_values"].cuda(), inp["src_ids"].cuda(), max_length=10, num_beams=3)
    assert m.transformer.training
    la2, ga2 = step(m, g)
    lb2, gb2 = step(m0, g)
    assert la == lb and la2 == lb2 and la2 == la
    assert torch.allclose(ga, gb, atol=1e-6, rtol=1e-5)
    assert torch.allclose(ga2, gb2, atol=1e-6, rtol=1e-5)


def test_generate_beam_argument_errors():
    m, g = _build("tiny_b", "fp32")
    inp = g["inputs"]
    pix, src = inp["pixel_values"].cuda(), inp["src_ids"].cuda()
    with pytest.raises(ValueError, match=r"`num_return_sequences` \(3\) has to be smaller or equal to `num_beams` \(2\)"):
        m.generate(pix, src, num_beams=2, num_return_sequences=3)
    with pytest.raises(ValueError, match="kv_cache"):
        m.generate(pix, src, num_beams=2, kv_cache=False)
    m.transformer.eval()
    m.generate(pix, src, max_length=8, num_beams=2)
    assert not m.transformer.training


def test_generate_num_beams_1_is_greedy():
    m, g = _build("tiny_b", "fp32")
    inp = g["inputs"]
    pix, src = inp["pixel_values"].cuda(), inp["src_ids"].cuda()
    a = m.generate(pix, src, max_length=12)
    b = m.generate(pix, src, max_length=12, num_beams=1)
    assert torch.equal(a, b)
