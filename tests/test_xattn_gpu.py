"""Cross-attention maps on the GPU: klab_t5_decode_attn_map against the exact fixtures and the per-element bound of
tests/xattn_ref.py (tests/test_xattn_cpu.py proves both on the CPU), the decoding session with maps against the same session
without them (bit-identical tokens and log-probabilities) and against the fixture recorded from the reference
(tests/golden/xattn.npz, make_xattn_goldens.py), and the arming rules of klab_engine_gen_set_attn."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import xattn_ref as X
from tests.helpers import GOLD
from tests.test_force_gpu import _model

pytestmark = pytest.mark.gpu

EOS = 1
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
MIDS = ("tiny_b.plain", "tiny_b.eos", "tiny_v11_a.plain")


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------------
def run_map(q_src, k_src, bias, groups, dtype, done=None, misalign=False):
    """one launch over R rows.  K lies as the engine's cross K/V does (k | v per key, the v half NaN: it is never read), the queries
    in rows of a larger pitch, the bias rows in a pitch of Lk + 5 with NaN behind them; the map has a margin row in front and
    behind and three margin columns, all NaN.  misalign: K starts one element off a 16-byte boundary (the scalar-load form)."""
    from klab_multimodalmodel_amd import ops
    q_div, kv_group = groups
    nq, H, dk = q_src.shape
    nk, _, Lk, _ = k_src.shape
    inner = H * dk
    kv = torch.full((nk, Lk, 2 * inner), float("nan"), dtype=dtype)
    kv[:, :, :inner] = k_src.transpose(1, 2).reshape(nk, Lk, inner).to(dtype)
    store = torch.zeros(kv.numel() + 8, dtype=dtype, device="cuda")
    kd = store[1:1 + kv.numel()] if misalign else store[:kv.numel()]
    kd.copy_(kv.reshape(-1))
    assert (kd.data_ptr() % 16 != 0) == misalign
    qd = torch.full((nq, inner + 8), float("nan"), dtype=dtype)
    qd[:, :inner] = q_src.reshape(nq, inner).to(dtype)
    qd = qd.cuda()
    bd = None
    if bias is not None:
        bd = torch.full((H, Lk + 5), float("nan"))
        bd[:, :Lk] = bias.float()
        bd = bd.cuda()
    dd = None if done is None else torch.tensor(done, dtype=torch.int32, device="cuda")
    out = torch.full((X.R + 2, Lk + 3), float("nan"), device="cuda")
    ops.decode_attn_map(qd, kd, out[1:], R=X.R, H=H, Lk=Lk, dk=dk, q_bstride=inner + 8, kv_bstride=Lk * 2 * inner, ldk=2 * inner,
                        out_bstride=Lk + 3, q_div=q_div, kv_group=kv_group, bias_row=bd, bias_ld=Lk + 5, done=dd)
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[0]).all() and torch.isnan(out[-1]).all() and torch.isnan(out[1:-1, Lk:]).all(), "a sentinel was overwritten"
    return out[1:-1, :Lk]


@pytest.mark.parametrize("kind,n", X.EXACT_KINDS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_map_kernel_is_exact_on_the_dyadic_fixtures(dtype, kind, n):
    """every probability is 1 / n on the chosen keys, the head mean of a power-of-two H is a dyadic number: torch.equal with the
    written-down map; rows marked done are exactly 0"""
    done = torch.tensor(X.DONE, dtype=torch.bool)
    for i, (H, dk, Lk, groups) in enumerate(X.exact_cases(kind)):
        for pos in range(3):
            q_src, k_src, bias, want = X.exact_operands(kind, n, H, dk, Lk, groups, pos)
            with_done = (i + pos) % 2 == 0
            got = run_map(q_src, k_src, bias, groups, DT[dtype], X.DONE if with_done else None, misalign=i % 3 == 0)
            if with_done:
                want = torch.where(done[:, None], torch.zeros_like(want), want)
            assert got.dtype == torch.float32 and torch.equal(got.double(), want), (kind, dtype, H, dk, Lk, groups, pos, with_done)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_map_kernel_random_operands_within_the_bound(dtype):
    """|map - float64| <= mean_h(P_h f_h) + 2 (H + 2) 2^-24 mean_h(P_h) per element (f_h: exact_ref.attn_f32_factor), every live
    row sums to 1 within 2 (Lk + H + 16) 2^-24, nothing is negative"""
    done = torch.tensor(X.DONE, dtype=torch.bool)
    for i, (H, dk, Lk, groups, with_bias) in enumerate(X.RANDOM_CASES):
        q_src, k_src, bias = X.random_operands(H, dk, Lk, groups, with_bias, i)
        q, k = X.per_row(q_src, k_src, groups)
        ref, P = X.head_mean_map(q, k, bias)
        bound = X.map_bound(q, k, P, Lk, dk)
        for with_done in (False, True):
            got = run_map(q_src, k_src, bias, groups, DT[dtype], X.DONE if with_done else None, misalign=i % 2 == 1).double()
            live = ~done if with_done else torch.ones_like(done)
            err = (got - ref).abs()[live]
            ratio = float((err / bound[live]).max())
            rowsum = float((got[live].sum(-1) - 1).abs().max())
            print(f"{dtype} H {H} dk {dk} Lk {Lk} {groups} bias {with_bias}: max err / bound {ratio:.3f}, |row sum - 1| {rowsum:.2e} "
                  f"(allowed {X.row_sum_bound(Lk, H):.2e})")
            assert (err <= bound[live]).all(), (dtype, H, dk, Lk, ratio)
            assert rowsum <= X.row_sum_bound(Lk, H) and (got >= 0).all()
            assert (got[~live] == 0).all()


def test_map_kernel_is_bit_reproducible():
    """no atomics, a fixed head order: two launches give the same bits"""
    H, dk, Lk, groups, with_bias = X.RANDOM_CASES[3]
    q_src, k_src, bias = X.random_operands(H, dk, Lk, groups, with_bias, 3)
    a = run_map(q_src, k_src, bias, groups, torch.bfloat16)
    b = run_map(q_src, k_src, bias, groups, torch.bfloat16)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_map_kernel_bad_arguments():
    """errors, and nothing is launched: the output keeps its sentinels"""
    from klab_multimodalmodel_amd import ops
    H, dk, Lk = 2, 8, 4
    q = torch.zeros(2, H * dk, device="cuda")
    k = torch.zeros(2, Lk, H * dk, device="cuda")
    out = torch.full((2, Lk), float("nan"), device="cuda")
    ok = dict(R=2, H=H, Lk=Lk, dk=dk, q_bstride=H * dk, kv_bstride=Lk * H * dk, ldk=H * dk, out_bstride=Lk)
    for bad in (dict(R=0), dict(H=0), dict(Lk=0), dict(q_div=0), dict(kv_group=0), dict(out_bstride=Lk - 1),
                dict(bias_row=torch.zeros(H, Lk, device="cuda"), bias_ld=Lk - 1)):
        with pytest.raises(ValueError):
            ops.decode_attn_map(q, k, out, **{**ok, **bad})
    for bad_dk in (4, 12, 256):
        with pytest.raises(NotImplementedError):
            ops.decode_attn_map(q, k, out, **{**ok, "dk": bad_dk})
    with pytest.raises(ValueError):
        ops.decode_attn_map(q, k.bfloat16(), out, **ok)  # q and k of two dtypes
    with pytest.raises(ValueError):
        ops.decode_attn_map(q.half(), k.half(), out, **ok)  # neither bf16 nor f32
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    ops.decode_attn_map(q, k, out, **ok)  # ... and the good call writes: zero scores, the uniform map
    torch.cuda.synchronize()
    assert (out == 1.0 / Lk).all()


# ---- 2. session and model --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gold():
    return (np.load(os.path.join(GOLD, "xattn.npz")), json.load(open(os.path.join(GOLD, "xattn.json"))),
            np.load(os.path.join(GOLD, "force.npz")))


def _meta(mid):
    return next(mm for mm in _gold()[1]["models"] if mm["id"] == mid)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                    b.view(torch.int32) if b.dtype == torch.float32 else b)


def _live_columns(seq, first_free=1):
    """bool [rows, L]: the columns of a map that hold an attention -- column p >= 1 until the row's first EOS at a position the
    session chose itself (>= first_free: an EOS inside a decoder prompt finishes nothing), that EOS's own column included"""
    hit = (seq == EOS) & (torch.arange(seq.shape[1], device=seq.device)[None] >= first_free)
    before = torch.cumsum(hit.long(), 1) - hit.long()
    live = before < 1
    live[:, 0] = False
    return live


def _check_maps(info, seq, m, first_free=1):
    """shape, the two entries that say where the image is, zeros where nothing attended, probabilities elsewhere"""
    att = info["cross_attention"]
    eng = m._engine
    nld, Le = m.main_cfg.num_decoder_layers, eng.n_img + eng.shape[1]
    assert att.dtype == torch.float32 and tuple(att.shape) == (seq.shape[0], nld, seq.shape[1], Le), (att.shape, seq.shape)
    assert info["image_tokens"] == eng.n_img and info["image_grid"] == (int(eng.n_img ** 0.5),) * 2
    assert info["image_grid"][0] ** 2 == eng.n_img
    live = _live_columns(seq, first_free)[:, None, :].expand(-1, nld, -1)
    assert (att[~live] == 0).all()
    s = att[live].double().sum(-1)
    assert (att >= 0).all() and float((s - 1).abs().max()) <= X.row_sum_bound(Le, m.main_cfg.num_heads)


@pytest.mark.parametrize("mid", MIDS)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_generate_is_bit_identical_with_maps(dtype, mid):
    """greedy, greedy behind the processors, sampling, best_of and a decoder prompt: asking for the maps changes no token and no
    log-probability"""
    name, variant = mid.rsplit(".", 1)
    m, (pix, src) = _model(name, dtype, variant)
    z = _gold()[2]
    prompt = torch.from_numpy(z[mid + ".p3.none.prompt"])
    procs = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    cases = [("greedy", dict(), None),
             ("greedy+logprobs", dict(return_logprobs=True), None),
             ("processors", dict(return_logprobs=True, min_new_tokens=3, **procs), None),
             ("sampling", dict(do_sample=True, num_return_sequences=3, top_k=20, temperature=0.9, return_logprobs=True), 11),
             ("sampling+processors", dict(do_sample=True, num_return_sequences=2, top_p=0.9, **procs), 12),
             ("best_of", dict(do_sample=True, best_of=4, num_return_sequences=2, top_k=20, return_logprobs=True), 13),
             ("best_of, no logprobs", dict(do_sample=True, best_of=3, num_return_sequences=1, top_k=20), 14),
             ("prompt", dict(decoder_input_ids=prompt, min_new_tokens=2), None),
             ("prompt+sampling", dict(decoder_input_ids=prompt, do_sample=True, num_return_sequences=2, top_k=20), 15)]
    for what, kw, seed in cases:
        if seed is not None:
            torch.manual_seed(seed)
        plain = m.generate(pix, src, max_length=10, **kw)
        if seed is not None:
            torch.manual_seed(seed)
        seq, info = m.generate(pix, src, max_length=10, return_cross_attention=True, **kw)
        if kw.get("return_logprobs"):
            assert _same(plain[0], seq), (mid, dtype, what)
            for key in ("token_logprobs", "scores", "lengths"):
                assert _same(plain[1][key], info[key]), (mid, dtype, what, key)
        else:
            assert _same(plain, seq), (mid, dtype, what)
            assert set(info) == {"cross_attention", "image_tokens", "image_grid"}, (what, set(info))
        _check_maps(info, seq, m, first_free=1 + prompt.shape[1] if "decoder_input_ids" in kw else 1)


def test_best_of_maps_follow_the_sequences():
    """with best_of the rows of the maps are gathered with the sequences' order: each returned row's map is the map of the full
    session's row that holds the same tokens"""
    m, (pix, src) = _model("tiny_v11_a", "fp32")
    kw = dict(max_length=10, do_sample=True, top_k=20, return_cross_attention=True, return_logprobs=True)
    torch.manual_seed(21)
    seq, info = m.generate(pix, src, best_of=4, num_return_sequences=2, **kw)
    torch.manual_seed(21)
    full, finfo = m.generate(pix, src, num_return_sequences=4, **kw)
    B = src.shape[0]
    assert full.shape[0] == 4 * B and seq.shape[0] == 2 * B
    for r in range(seq.shape[0]):
        b = r // 2
        rows = [j for j in range(4 * b, 4 * b + 4) if torch.equal(full[j], seq[r]) and
                torch.equal(finfo["token_logprobs"][j], info["token_logprobs"][r])]
        assert rows, r
        assert any(torch.equal(finfo["cross_attention"][j], info["cross_attention"][r]) for j in rows), r


def _session(m, pix, src, mode, n, max_length, buf=None, steps=None, **kw):
    """a session driven by hand; buf: armed in front of gen_begin"""
    cfg = m.main_cfg
    B = src.shape[0]
    tgt = torch.full((B, max_length - 1), cfg.pad_token_id, dtype=torch.int64, device="cuda")
    eng = m._engine_for(pix, src, tgt)
    m.transformer.eval()
    with torch.no_grad():
        eng.forward(pix, src, tgt, training=0, seed=m._seed_base, want_grad=False)
        gen = eng.gen_cfg(mode, n, max_length, cfg.eos_token_id, cfg.pad_token_id, **kw)
        ws = torch.empty(eng.gen_workspace_bytes(gen), dtype=torch.uint8, device="cuda")
        if buf is not None:
            eng.gen_set_attn(buf)
        eng.gen_begin(gen, ws)
        for t in range(1, (max_length - 1) if steps is None else steps + 1):
            eng.gen_step(t, ws)
        seq = eng.gen_result(ws, n, max_length if steps is None else steps + 1)[0]
    torch.cuda.synchronize()
    return eng, gen, ws, seq


def test_arming_is_one_shot_and_sized():
    m, (pix, src) = _model("tiny_b", "fp32")
    cfg = m.main_cfg
    B, n, ml = src.shape[0], 2, 8
    eng, gen, ws, seq = _session(m, pix, src, "sample", n, ml, seed=5, top_k=20)
    Le, nld = eng.n_img + eng.shape[1], cfg.num_decoder_layers
    need = eng.gen_attn_bytes(gen)
    assert need == nld * B * n * ml * Le * 4
    assert need == eng.gen_attn_bytes(eng.gen_cfg("pick", n, ml, cfg.eos_token_id, cfg.pad_token_id, want_logprobs=True))
    assert need == eng.gen_attn_bytes(eng.gen_cfg("force", n, ml, cfg.eos_token_id, cfg.pad_token_id, want_logprobs=True))
    beam = eng.gen_cfg("beam", n, ml, cfg.eos_token_id, cfg.eos_token_id)
    assert eng.gen_attn_bytes(beam) == 0 and eng.gen_workspace_bytes(beam) > 0
    assert eng.gen_attn_bytes(eng.gen_cfg("sample", n, ml, cfg.eos_token_id, cfg.pad_token_id, temperature=0.0)) == 0  # refused settings
    # the maps are the caller's: the workspace is what it is without them
    sizes = [eng.gen_workspace_bytes(eng.gen_cfg(mode, n, ml, cfg.eos_token_id, cfg.pad_token_id, want_logprobs=lp))
             for mode, lp in (("pick", False), ("pick", True), ("sample", False), ("sample", True))]
    buf = torch.full((need // 4,), 7.0, device="cuda")
    eng.gen_set_attn(buf)
    assert sizes == [eng.gen_workspace_bytes(eng.gen_cfg(mode, n, ml, cfg.eos_token_id, cfg.pad_token_id, want_logprobs=lp))
                     for mode, lp in (("pick", False), ("pick", True), ("sample", False), ("sample", True))]
    bws = torch.empty(eng.gen_workspace_bytes(beam), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        eng.gen_begin(beam, bws)  # beam search carries no maps
    eng.gen_begin(beam, bws)  # ... and the refused begin left nothing armed
    torch.cuda.synchronize()
    assert (buf == 7.0).all()
    eng.gen_set_attn(buf[:need // 4 - 1])
    with pytest.raises(ValueError):
        eng.gen_begin(gen, ws)  # one element short
    eng.gen_begin(gen, ws)  # consumed by the failure: this session has no maps
    eng.gen_step(1, ws)
    torch.cuda.synchronize()
    assert (buf == 7.0).all()
    eng.gen_set_attn(buf)
    eng.gen_set_attn(None)  # disarmed
    eng.gen_begin(gen, ws)
    torch.cuda.synchronize()
    assert (buf == 7.0).all()
    with pytest.raises(ValueError):
        eng.gen_set_attn(buf.double())
    with pytest.raises(ValueError):
        eng.gen_set_attn(buf.view(2, -1)[:, 1:])  # not contiguous


def test_a_later_session_leaves_the_old_maps_alone():
    """maps are a property of one session: the next one, begun without arming, writes nothing to the buffer of the last"""
    m, (pix, src) = _model("tiny_b", "fp32")
    B, n, ml = src.shape[0], 2, 8
    eng, gen, ws, seq = _session(m, pix, src, "sample", n, ml, seed=5, top_k=20)
    buf = torch.full((eng.gen_attn_bytes(gen) // 4,), float("nan"), device="cuda")
    eng, gen, ws, seq2 = _session(m, pix, src, "sample", n, ml, buf=buf, seed=5, top_k=20)
    assert torch.equal(seq, seq2)
    maps = buf.view(m.main_cfg.num_decoder_layers, B * n, ml, -1)
    assert not torch.isnan(maps).any() and (maps[:, :, 0] == 0).all()  # cleared by gen_begin, column 0 stays 0
    live = _live_columns(seq2)
    sums = maps.permute(1, 0, 2, 3)[live[:, None].expand(-1, maps.shape[0], -1)].double().sum(-1)
    assert float((sums - 1).abs().max()) <= X.row_sum_bound(maps.shape[-1], m.main_cfg.num_heads)
    buf.fill_(7.0)
    _session(m, pix, src, "sample", n, ml, seed=6, top_k=20)
    _session(m, pix, src, "pick", 1, ml)
    assert (buf == 7.0).all()


@pytest.mark.parametrize("mid", MIDS)
def test_score_maps_match_the_reference(mid):
    """fp32 engine against HF's float64 cross_attentions of the same candidates: max |error| <= 4 d32 + 2^-20 over every live
    position, d32 = what the reference's own fp32 run differs from its float64 run by (xattn.json; engine and torch sum every
    product along the depth in different orders: an independent error of the same size, hence the factor).  Measured on the
    MI355X: see DESIGN.md section 5."""
    z, _, force = _gold()
    name, variant = mid.rsplit(".", 1)
    m, (pix, src) = _model(name, "fp32", variant)
    cand = torch.from_numpy(force[mid + ".cand"])
    B, N, L = cand.shape
    want = torch.from_numpy(z[mid + ".cand_maps"])
    plain = m.score(pix, src, cand)
    out = m.score(pix, src, cand, return_cross_attention=True)
    for key in plain:
        assert _same(plain[key], out[key]), key
    att = out["cross_attention"].cpu()
    nld, Le = want.shape[2], want.shape[4]
    assert att.dtype == torch.float32 and tuple(att.shape) == (B, N, nld, L, Le)
    assert out["image_tokens"] == _meta(mid)["image_tokens"] and out["image_grid"][0] ** 2 == out["image_tokens"]
    live = X.live_labels(cand, EOS)[:, :, None, :].expand(-1, -1, nld, -1)
    assert live.any() and (~live).any()
    assert (att[~live] == 0).all()  # exactly 0 after a row's first EOS
    err = float((att.double() - want)[live].abs().max())
    d32 = _meta(mid)["d32"]
    print(f"{mid}: score maps vs float64 reference {err:.3e}; d32 {d32:.3e}; allowed {4 * d32 + 2.0 ** -20:.3e}")
    assert err <= 4 * d32 + 2.0 ** -20, (mid, err, d32)


@pytest.mark.parametrize("mid", MIDS)
def test_score_maps_bf16_parity(mid):
    """the project's parity criterion for the bf16 engine, per (row, layer, position): cosine >= 0.99 with the reference"""
    z, _, force = _gold()
    name, variant = mid.rsplit(".", 1)
    m, (pix, src) = _model(name, "bf16", variant)
    cand = torch.from_numpy(force[mid + ".cand"])
    want = torch.from_numpy(z[mid + ".cand_maps"])
    nld = want.shape[2]
    out = m.score(pix, src, cand, return_cross_attention=True)
    att = out["cross_attention"].cpu().double()
    live = X.live_labels(cand, EOS)[:, :, None, :].expand(-1, -1, nld, -1)
    assert (att[~live] == 0).all()
    cos = (att * want).sum(-1) / (att.norm(dim=-1) * want.norm(dim=-1) + 1e-30)
    worst = float(cos[live].min())
    print(f"{mid}: bf16 score maps, worst cosine {worst:.5f}")
    assert worst >= 0.99, (mid, worst)


@pytest.mark.parametrize("mid", MIDS)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_greedy_maps_match_the_reference(dtype, mid):
    """generate's maps on the model's own greedy ids against the reference's maps on ITS greedy ids, to the bounds of the two score
    tests; column p holds the attention that predicted the token of position p, the reference's label p - 1, and is comparable
    where the two decoders were fed the same tokens, ids[:, :p].  The fp32 engine decodes the reference's ids on all three
    fixtures (asserted).  The bf16 engine does on tiny_b; on tiny_v11_a its row 0 leaves them at position 5 (34 5 83 34 | 5 against
    the reference's 63, on the MI355X), so there the columns up to the first difference are compared, and they must be at least
    half of all live columns."""
    z, meta, _ = _gold()
    name, variant = mid.rsplit(".", 1)
    m, (pix, src) = _model(name, dtype, variant)
    ids = torch.from_numpy(z[mid + ".greedy_ids"])
    want = torch.from_numpy(z[mid + ".greedy_maps"])
    seq, info = m.generate(pix, src, max_length=meta["max_length"], return_cross_attention=True)
    seq = seq.cpu()
    if dtype == "fp32":
        assert torch.equal(seq, ids), (mid, dtype, seq, ids)
    assert seq.shape == ids.shape, (mid, dtype, seq, ids)
    att = info["cross_attention"].cpu().double()
    assert (att[:, :, 0] == 0).all()
    assert (att[~_live_columns(seq)[:, None].expand(-1, want.shape[1], -1)] == 0).all()
    same_input = torch.cumsum((seq != ids).long(), 1) - (seq != ids).long() < 1  # column p: seq[:, :p] == ids[:, :p]
    live = (_live_columns(ids) & same_input)[:, None, 1:].expand(-1, want.shape[1], -1)
    assert 2 * int(live.sum()) >= int(_live_columns(ids).sum()) * want.shape[1], (mid, dtype, seq, ids)
    got = att[:, :, 1:]
    if dtype == "fp32":
        err = float((got - want)[live].abs().max())
        d32 = _meta(mid)["d32"]
        print(f"{mid}: greedy maps vs float64 reference {err:.3e}; d32 {d32:.3e}; allowed {4 * d32 + 2.0 ** -20:.3e}")
        assert err <= 4 * d32 + 2.0 ** -20, (mid, err, d32)
    else:
        cos = (got * want).sum(-1) / (got.norm(dim=-1) * want.norm(dim=-1) + 1e-30)
        worst = float(cos[live].min())
        print(f"{mid}: bf16 greedy maps, worst cosine {worst:.5f}")
        assert worst >= 0.99, (mid, worst)
