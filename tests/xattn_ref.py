"""Head-mean decode cross-attention in plain torch, float64 (CPU): the references of tests/test_xattn_cpu.py and
tests/test_xattn_gpu.py.  oracle/swin_t5_oracle.py forms the same probabilities inside t5_attention but does not return them.

head_mean_map: what klab_t5_decode_attn_map computes for one query row per decoding row, from per-row operands.
decoder_cross_attention: the T5 decoder (HF/t5 T5Stack with is_decoder) teacher-forced on labels over a given encoder output, on
the model's own weights, returning only mean_h softmax(q_h k_h^T) of every layer's EncDecAttention: HF's `cross_attentions` of
output_attentions=True averaged over the heads.  Position l of the result is the attention of the query at decoder position l
(input: the start token for l = 0, else label l - 1), i.e. the attention that predicts label l; the causal mask makes it the
same numbers a step-by-step decode over a K/V cache produces.  Both feed-forward forms (ReLU; gated gelu_new of T5 v1.1) are
restated, the one in use read off the weights' names.  One detail is HF's and not float64: T5LayerNorm takes the mean of squares
in float32 whatever the model's dtype (HF/t5:65), so the float64 run of the reference does, and so does this file."""
import math

import torch
import torch.nn.functional as F

from oracle import swin_t5_oracle as O

U24 = 2.0 ** -24


def head_mean_map(q, k, bias=None, done=None):
    """q [R, H, dk], k [R, H, Lk, dk] (row r's own query and keys), bias [H, Lk] or None, done bool [R] or None ->
    (map [R, Lk] = mean_h softmax_j(q_h . k_hj + bias_hj), 0 for done rows; P [R, H, Lk]), in the operands' dtype"""
    s = torch.einsum("rhd,rhjd->rhj", q, k)
    if bias is not None:
        s = s + bias[None]
    P = torch.softmax(s, -1)
    m = P.sum(1) * (1.0 / P.shape[1])
    if done is not None:
        m = torch.where(done[:, None], torch.zeros_like(m), m)
        P = torch.where(done[:, None, None], torch.zeros_like(P), P)
    return m, P


def map_bound(q, k, P, Lk, dk):
    """per-element bound of an f32 evaluation of head_mean_map against the float64 one, [R, Lk]: every probability carries
    tests/exact_ref.py's attn_f32_factor f_h as a relative error, the H-term head sum and the scaling by 1 / H add
    2 (H + 2) 2^-24 relative to the mean:  mean_h(P_h f_h) + 2 (H + 2) 2^-24 mean_h(P_h)"""
    H = P.shape[1]
    f = 2.0 * U24 * ((dk + 2) * torch.einsum("rhd,rhjd->rhj", q.abs(), k.abs()) + Lk + 16)
    return (P * f).mean(1) + 2.0 * (H + 2) * U24 * P.mean(1)


def row_sum_bound(Lk, H):
    """|sum_j map[r, j] - 1| of a live row: Lk additions of probabilities that are each off by a few ulp, H heads, the normaliser"""
    return 2.0 * (Lk + H + 16) * U24


def _rmsnorm(x, w, eps):
    var = x.to(torch.float32).pow(2).mean(-1, keepdim=True)  # (HF/t5:65: float32 for every model dtype)
    return w * (x * torch.rsqrt(var + eps))


def _gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


def decoder_cross_attention(sd, cfg, enc_out, labels, dtype=torch.float64):
    """sd: the main model's state dict (HF names; `shared.weight` is the decoder's embedding); cfg: anything with HF's T5 field
    names (num_heads, num_decoder_layers, layer_norm_epsilon, relative_attention_num_buckets, relative_attention_max_distance,
    decoder_start_token_id); enc_out [R, Le, d]; labels int64 [R, L].  Returns [R, n_dec_layers, L, Le] in `dtype`."""
    w = {n: t.to(dtype) for n, t in sd.items() if n.startswith("decoder.") or n == "shared.weight"}
    H, eps = cfg.num_heads, cfg.layer_norm_epsilon
    R, L = labels.shape
    enc = enc_out.to(dtype)
    ids = torch.cat([torch.full((R, 1), cfg.decoder_start_token_id, dtype=torch.int64), labels[:, :-1]], 1)
    x = F.embedding(ids, w["shared.weight"])
    bias = O.t5_position_bias(w["decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], L, L, False, cfg).to(dtype)
    keep = torch.tril(torch.ones(L, L, dtype=torch.bool))

    def heads(t):
        return t.view(t.shape[0], t.shape[1], H, -1).transpose(1, 2)

    maps = []
    for i in range(cfg.num_decoder_layers):
        bp = f"decoder.block.{i}."
        n = _rmsnorm(x, w[bp + "layer.0.layer_norm.weight"], eps)
        a = bp + "layer.0.SelfAttention."
        s = heads(F.linear(n, w[a + "q.weight"])) @ heads(F.linear(n, w[a + "k.weight"])).transpose(2, 3) + bias
        p = torch.softmax(s.masked_fill(~keep, float("-inf")), -1)
        x = x + F.linear((p @ heads(F.linear(n, w[a + "v.weight"]))).transpose(1, 2).reshape(R, L, -1), w[a + "o.weight"])
        n = _rmsnorm(x, w[bp + "layer.1.layer_norm.weight"], eps)
        a = bp + "layer.1.EncDecAttention."
        p = torch.softmax(heads(F.linear(n, w[a + "q.weight"])) @ heads(F.linear(enc, w[a + "k.weight"])).transpose(2, 3), -1)
        maps.append(p.mean(1))
        x = x + F.linear((p @ heads(F.linear(enc, w[a + "v.weight"]))).transpose(1, 2).reshape(R, L, -1), w[a + "o.weight"])
        n = _rmsnorm(x, w[bp + "layer.2.layer_norm.weight"], eps)
        f = bp + "layer.2.DenseReluDense."
        if f + "wi_0.weight" in w:
            mid = _gelu_new(F.linear(n, w[f + "wi_0.weight"])) * F.linear(n, w[f + "wi_1.weight"])
        else:
            mid = F.relu(F.linear(n, w[f + "wi.weight"]))
        x = x + F.linear(mid, w[f + "wo.weight"])
    return torch.stack(maps, 1)


# ---- the kernel's cases (shared by the CPU proof and the GPU test) ----------------------------------------------------------------
# R = 6 decoding rows; row r reads query row r // q_div and the keys of sample r // kv_group.  The exact fixtures are
# tests/exact_ref.py's AttnFixture at Lq = 3, one launch per query position (the position bias row is shared by the rows of a
# launch, as in a decode step): position 0 chooses from key 0 on, position 2 from the last key on, position 1 from a key that
# walks with the head, so that the heads of a row choose different keys and the head sum is not a sum of equal terms.
R = 6
DONE = (0, 1, 0, 0, 1, 0)
EXACT_KINDS = (("onehot", 1), ("q0", 4), ("k0", 2), ("onehot_nobias", 1))
EXACT_H = (1, 2, 4, 8, 16)
EXACT_DK = (8, 16, 64, 128)
EXACT_LK = (1, 63, 64, 65, 129, 577)
GROUPS = ((1, 1), (3, 1), (1, 3), (3, 3))  # (q_div, kv_group)
RANDOM_CASES = [(H, dk, Lk, GROUPS[i % 4], bool(i & 1)) for i, (H, dk, Lk) in enumerate(
    [(6, 16, 63), (6, 64, 129), (12, 8, 65), (12, 64, 577), (32, 32, 64), (32, 128, 129), (6, 128, 1), (12, 16, 577)])]


def nobias_allowed(Lk, dk):
    """exact_ref.sign_codes needs the key index, and a parity bit, inside the head dim"""
    return max(1, (Lk - 1).bit_length()) + 1 <= dk


def exact_cases(kind):
    """(H, dk, Lk, (q_div, kv_group)) for every dk x Lk, H and the grouping cycling through their values (5 and 4 against 24 cases:
    every H meets every dk and most Lk, every grouping every dk)"""
    out = []
    for i, (dk, Lk) in enumerate((dk, Lk) for dk in EXACT_DK for Lk in EXACT_LK):
        if kind == "onehot_nobias" and not nobias_allowed(Lk, dk):
            continue
        out.append((EXACT_H[i % 5], dk, Lk, GROUPS[(i + i // 6) % 4]))
    return out


def exact_operands(kind, n, H, dk, Lk, groups, pos):
    """per-row float64 operands of one launch from the fixture: q_src [R // q_div, H, dk], k_src [R // kv_group, H, Lk, dk],
    bias [H, Lk] or None, and the written-down map [R, Lk] (done rows included: the caller zeroes them)"""
    from tests.exact_ref import attn_fixture
    q_div, kv_group = groups
    g = max(q_div, kv_group)
    f = attn_fixture(kind, R // g, H, 3, Lk, dk, False, n)
    q_src = f.q[:, :, pos].repeat_interleave(g // q_div, 0)
    k_src = f.k.repeat_interleave(g // kv_group, 0)
    bias = None if f.bias is None else f.bias[:, pos]
    want = (f.P[:, :, pos].sum(1) * (1.0 / H)).repeat_interleave(g, 0)
    return q_src, k_src, bias, want


def per_row(q_src, k_src, groups):
    """the operands as each of the R rows sees them: q [R, H, dk], k [R, H, Lk, dk]"""
    return q_src.repeat_interleave(groups[0], 0), k_src.repeat_interleave(groups[1], 0)


def random_operands(H, dk, Lk, groups, with_bias, seed=0):
    """randn q and K rounded to bf16 (float64 holds them), a position-bias row of a few units or None"""
    g = torch.Generator().manual_seed(7000 + seed)
    q_src = torch.randn(R // groups[0], H, dk, generator=g).to(torch.bfloat16).double()
    k_src = torch.randn(R // groups[1], H, Lk, dk, generator=g).to(torch.bfloat16).double()
    bias = (2.0 * torch.randn(H, Lk, generator=g)).float().double() if with_bias else None
    return q_src, k_src, bias


# ---- the golden models ---------------------------------------------------------------------------------------------------------------
def golden_weights(mid):
    """(the main model's state dict, its T5Config with HF's field names) of the golden model <name>.<variant>"""
    import os

    import numpy as np

    from tests.helpers import GOLD, load_golden
    name, variant = mid.rsplit(".", 1)
    if name.startswith("tiny_v11"):
        from tests.v11_helpers import configs, load_v11
        g = load_v11(name)
        return g["sds"]["main"], configs(g)[2]
    from klab_multimodalmodel_amd.engine import T5Config
    g = load_golden(name)
    sd = dict(g["sds"]["main"])
    if variant == "eos":
        sd["shared.weight"] = sd["shared.weight"].clone()
        sd["shared.weight"][1] = torch.from_numpy(np.load(os.path.join(GOLD, "beam.npz"))[f"{name}.eos_row"])
    return sd, T5Config.from_dict(g["meta"]["t5_config"])


def live_labels(labels, eos_id):
    """bool [..., L]: the label positions through each row's first EOS (what follows it is not compared)"""
    hit = labels == eos_id
    return (torch.cumsum(hit.long(), -1) - hit.long()) < 1
