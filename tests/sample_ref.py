"""Torch restatement of HF's sampling warpers (transformers/generation/logits_process.py: TemperatureLogitsWarper,
TopKLogitsWarper, TopPLogitsWarper, built and ordered as generation/utils.py does for do_sample=True, num_beams=1) and the
fp64 checks the sampling tests apply to klab_sample_rows."""
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
