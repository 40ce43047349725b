"""Torch restatement of HF's sampling warpers (transformers/generation/logits_process.py: TemperatureLogitsWarper,
TopKLogitsWarper, TopPLogitsWarper, built and ordered as generation/utils.py does for do_sample=True, num_beams=1) and the
fp64 checks the sampling tests apply to klab_sample_rows."""
import functools

import torch


def hf_warp(logits, temperature=1.0, top_k=50, top_p=1.0):
    """the processed scores HF's `_sample` hands to softmax: fp32 logits -> temperature -> top-k -> top-p (-inf = removed)"""
    scores = logits.float()
    if temperature != 1.0:
        scores = scores / temperature
    if top_k != 0:
        k = min(max(top_k, 1), scores.size(-1))
        scores = scores.masked_fill(scores < torch.topk(scores, k)[0][..., -1, None], -float("inf"))
    if top_p < 1.0:
        sorted_logits, sorted_indices = torch.sort(scores, descending=False)
        cumulative_probs = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
        remove = cumulative_probs <= (1 - top_p)
        remove[..., -1:] = 0
        remove = remove.scatter(1, sorted_indices, remove)
        scores = scores.masked_fill(remove, -float("inf"))
    return scores


def boundary_tokens(logits, temperature, top_k, top_p, tol=1e-5):
    """bool [rows, V]: tokens whose kept / removed status may legitimately differ between HF's rule and the kernel's -- tied
    exactly with another token at the k-th value or at the top-p boundary, or whose strictly-larger mass lies within tol of
    top_p (fp64 from the fp32 scores)"""
    scores = logits.float()
    if temperature != 1.0:
        scores = scores / temperature
    V = scores.size(-1)
    out = torch.zeros_like(scores, dtype=torch.bool)
    kept = torch.ones_like(out)
    if top_k != 0 and top_k < V:
        kth = torch.topk(scores, top_k)[0][..., -1, None]
        out |= (scores == kth) & ((scores == kth).sum(-1, keepdim=True) > 1)
        kept = scores >= kth
    if top_p < 1.0:
        s64 = scores.double().masked_fill(~kept, -float("inf"))
        p = torch.softmax(s64, -1)
        for r in range(s64.shape[0]):
            sv, si = torch.sort(s64[r], descending=True)
            _, inv, cnt = torch.unique_consecutive(sv, return_inverse=True, return_counts=True)
            gmass = torch.zeros(len(cnt), dtype=torch.float64).index_add_(0, inv, p[r][si])
            above = (gmass.cumsum(0) - gmass)[inv]  # mass strictly above each sorted token
            gm = gmass[inv]
            # near the boundary, or a tie group the boundary falls inside (HF's sort splits it; the kernel keeps it whole)
            flag = ((above - top_p).abs() <= tol) | ((cnt[inv] > 1) & (above < top_p + tol) & (above + gm >= top_p - tol))
            out[r, si] |= flag & kept[r, si]
    return out


def inverse_cdf(warped, u):
    """fp64: over the kept tokens (warped > -inf) in ascending id, the smallest id whose running probability exceeds u, and
    the distance from u to the nearest CDF step of that row"""
    p = torch.softmax(warped.double(), -1)
    cdf = p.cumsum(-1)
    cdf = cdf / cdf[:, -1:]
    u = u.double().view(-1, 1)
    tok = (cdf > u).long().argmax(-1)
    steps = torch.where(p > 0, cdf, torch.full_like(cdf, 2.0))
    dist = (steps - u).abs().min(-1)[0]
    return tok, dist


# ---- the kernel's own rule and a fixture on which it has no boundary cases (tests/test_sample_exact_gpu.py) -----------------------------
GROUPS = (1, 2, 1, 3, 1, 1, 1, 1, 1, 1)  # tokens per level; level i scores -0.5 i
SAMPLE_VOCABS = (5, 33, 1000, 1057, 32768)
TEMPERATURES = (0.5, 1.0, 2.0)
U_HIGH = 1.0 - 2.0 ** -24


def scaled(logits, temperature):
    """f32 logits / temperature, a true f32 division (the kernel's and HF's `scores / temperature`)"""
    x = logits.float()
    return x / torch.full_like(x, temperature)


def kept_reference(logits, temperature, top_k, top_p, mut=None):
    """bool [rows, V]: csrc/sample.hip's stated rule in fp64 over the f32 scores.  top-k keeps every score >= the k-th largest (a tie
    at the k-th value stays whole); over the softmax of those, token i stays iff the mass of the kept tokens with a STRICTLY larger
    score is < top_p, and the arg-max always stays; top_p >= 1 removes nothing.  A -inf score is never kept."""
    s = scaled(logits, temperature).double()
    V = s.shape[-1]
    kept = s > -float("inf")
    if 0 < top_k < V:
        kth = torch.sort(s, -1, descending=True)[0][:, top_k - 1:top_k]
        kept &= s >= kth
        if mut == "tie group split at the k-th value":
            order = torch.sort(s, dim=-1, descending=True, stable=True)[1]
            kept = torch.zeros_like(kept).scatter(1, order[:, :top_k], True) & (s > -float("inf"))
    if top_p < 1.0:
        p = torch.softmax(s.masked_fill(~kept, -float("inf")), -1)
        if mut == "kept rule with <=":
            above = ((s[:, None, :] >= s[:, :, None]) * p[:, None, :]).sum(-1) - p  # peers of a tie group count as above
        else:
            above = _above_sorted(s, p)
        kept &= (above < top_p) | (s == s.max(-1, keepdim=True)[0])
    return kept


def _above_sorted(s, p):
    """the mass strictly above every token, by a sort (large vocabularies)"""
    out = torch.empty_like(p)
    for r in range(s.shape[0]):
        sv, si = torch.sort(s[r], descending=True)
        _, inv, cnt = torch.unique_consecutive(sv, return_inverse=True, return_counts=True)
        gmass = torch.zeros(len(cnt), dtype=torch.float64).index_add_(0, inv, p[r][si])
        out[r, si] = (gmass.cumsum(0) - gmass)[inv]
    return out


def level_count(V):
    """(groups, m): the leading tie groups that leave at least one background token"""
    groups = []
    for n in GROUPS:
        if sum(groups) + n > min(13, V - 1):
            break
        groups.append(n)
    return tuple(groups), sum(groups)


def _background(n, bf16):
    """n values <= -40, descending from -40; pairwise distinct, and exact in bf16 when bf16 (which has about 15 700 such values: a
    longer list repeats them from its 3rd on)"""
    if not bf16:
        return -40.0 - 0.25 * torch.arange(n, dtype=torch.float64)
    vals, step, v = [], 0.25, 40.0
    while len(vals) < n and v < 2.0 ** 120:
        vals.append(-v)
        v += step
        if v >= 2.0 * (step * 128):  # 128 values per binade
            step *= 2
    out = torch.tensor(vals, dtype=torch.float64)
    while len(out) < n:
        out = torch.cat((out, out[2:2 + n - len(out)]))
    return out


@functools.lru_cache(maxsize=None)
def sample_fixture(V, dn):
    """x [8, V] fp64, exact in the dtype.  m level tokens (tie groups GROUPS, level i at -0.5 i) over V - m background values <= -40.
    Rows 0-3 differ in where the level tokens sit: ids 0..m-1, ids V-m..V-1 (ascending score), around the edge between ids 31 and
    32 (the edge between two threads), at random.  The lowest and the highest background id hold the two largest background
    values (-40, -40.25), whose probability stays a normal f32 at every temperature used, so that the lowest and highest kept ids
    can be drawn.  Rows 4-7 are rows 0-3 with up to 5 background tokens from the middle at -inf, as a processor leaves them."""
    groups, m = level_count(V)
    g = torch.Generator().manual_seed(V)
    lev = torch.cat([torch.full((n,), -0.5 * i, dtype=torch.float64) for i, n in enumerate(groups)])
    bg = _background(V - m, dn == "bf16")
    if len(bg) > 2:
        mid = bg[2:][torch.randperm(len(bg) - 2, generator=g)]
        bg = torch.cat((bg[:1], mid, bg[1:2]))
    start = max(0, min(32 - m // 2, V - m))
    places = [torch.arange(m), torch.arange(V - m, V).flip(0), torch.arange(start, start + m), torch.randperm(V, generator=g)[:m]]
    x = torch.empty(8, V, dtype=torch.float64)
    for r, ids in enumerate(places):
        mask = torch.zeros(V, dtype=torch.bool)
        mask[ids] = True
        x[r, ids] = lev
        x[r, ~mask] = bg
        x[r + 4] = x[r]
        rest = torch.nonzero(~mask).flatten()
        x[r + 4, rest[len(rest) // 2:len(rest) // 2 + min(5, len(rest) - 2)]] = -float("inf")
    return x


def sample_settings(V, dn, temperatures=TEMPERATURES):
    """[(temperature, top_k, top_p, plain)].  plain: top_k from {0, 1, 4, m, V, V+5} unless its k-th value lies inside a tie group,
    top_p from {1, 0} and the midpoint of the mass interval of every singleton level of mass > 4e-3 -- on these HF's rule and the
    kernel's agree (the CPU test).  Not plain: a k inside a tie group, V-2 (beyond the finite scores of rows 4-7) and a top_p a
    quarter into the interval of a tie group of mass > 4e-3: the kernel's rule keeps the group whole."""
    groups, m = level_count(V)
    x = sample_fixture(V, dn)[:1]
    ends = set(torch.tensor(groups).cumsum(0).tolist())
    ks = [(k, True) for k in (0, 1, 4, m, V, V + 5) if k == 0 or k >= m or k in ends]
    ks += [(k, False) for k in (2, 5, 6) if k < m and k not in ends] + ([(V - 2, False)] if V >= 33 else [])
    out = []
    for t in temperatures:
        for k, plain_k in ks:
            s = scaled(x, t).double()
            kept = kept_reference(x, t, k, 1.0)
            p = torch.softmax(s.masked_fill(~kept, -float("inf")), -1)[0]
            ps = [(1.0, True), (0.0, True)]
            above = 0.0
            for i, n in enumerate(groups):
                ids = list(range(sum(groups[:i]), sum(groups[:i + 1])))
                mass = float(p[ids].sum())
                if mass > 4e-3 and bool(kept[0, ids].all()):
                    ps.append((above + 0.5 * mass, True) if n == 1 else (above + 0.25 * mass, False))
                above += mass
            out += [(t, k, float(torch.tensor(tp, dtype=torch.float32)), plain_k and plain_p) for tp, plain_p in ps]
    return out


def draw_points(logits, temperature, kept, mut=None):
    """[(row, u, token)]: draws whose outcome does not hang on f32 rounding.  Over the kept tokens in ascending id with the fp64
    softmax: u = 0 draws the lowest kept id; the midpoint of every CDF step wider than 1e-3 draws that step's token; u = 1 - 2^-24
    draws the last token with probability, where the CDF before it is more than 1e-5 below u and every kept id after it has
    probability 0 in f32 (its score more than 110 below the maximum)."""
    s = scaled(logits, temperature).double().masked_fill(~kept, -float("inf"))
    rel = s - s.max(-1, keepdim=True)[0]
    p = torch.softmax(s, -1)
    if mut == "descending ids":
        p = p.flip(-1)
    cdf = p.cumsum(-1)
    cdf = cdf / cdf[:, -1:]
    out = []
    for r in range(s.shape[0]):
        ids = torch.nonzero(kept[r]).flatten()
        if float(rel[r, ids[0]]) >= -85.0:
            out.append((r, 0.0, int(ids[0])))
        before = cdf[r] - p[r] / p[r].sum()
        for j in torch.nonzero(cdf[r] - before > 1e-3).flatten().tolist():
            out.append((r, float(0.5 * (before[j] + cdf[r, j])), (s.shape[1] - 1 - j) if mut == "descending ids" else j))
        if mut != "descending ids":
            t = int((cdf[r] > U_HIGH).long().argmax())
            later = ids[ids > t]
            if float(before[t]) < U_HIGH - 1e-5 and bool((rel[r, later] < -110.0).all()):
                out.append((r, U_HIGH, t))
    return out
