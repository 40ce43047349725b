"""Float64 restatement of the per-token log-probabilities of generate(return_logprobs=True) and of the sequence scores made of
them (HF: generate(output_scores=True, return_dict_in_generate=True) + compute_transition_scores(normalize_logits=True)).

The transition score of a step is log_softmax(s)[token], s the processed score row the step chose from: for greedy decoding the
logits after the logits processors (tests/logits_proc_ref.py), for sampling after processors, temperature, top-k and top-p.
The kept set of sampling is restated by klab_sample_rows' own documented rule (include/klab_mm.h), which is HF's except that a
tie at the top-p boundary stays whole: token i stays iff the softmax mass of the top-k-kept tokens with a strictly larger score
is < top_p."""
import numpy as np
import torch


def warped_scores(logits, temperature=1.0, top_k=0, top_p=1.0):
    """(scores float64 [rows, V] with -inf = removed, margin): the fp32 scores logits / temperature (HF and the kernel divide in
    fp32), filtered in float64.  margin = the smallest |mass strictly above a token - top_p| over all tokens (inf without
    top-p): a fixture whose margin is tiny could legitimately fall on either side in fp32"""
    s = (logits.float() / temperature).double() if temperature != 1.0 else logits.double()
    V = s.shape[-1]
    if top_k > 0 and top_k < V:
        kth = torch.topk(s, top_k)[0][..., -1, None]
        s = s.masked_fill(s < kth, -float("inf"))
    margin = float("inf")
    if top_p < 1.0:
        p = torch.softmax(s, -1)
        out = s.clone()
        for r in range(s.shape[0]):
            sv, si = torch.sort(s[r], descending=True)
            _, inv, cnt = torch.unique_consecutive(sv, return_inverse=True, return_counts=True)
            gmass = torch.zeros(len(cnt), dtype=torch.float64).index_add_(0, inv, p[r][si])
            above = (gmass.cumsum(0) - gmass)[inv]  # mass strictly above each sorted token
            keep = above < top_p
            keep[0] = True
            fin = torch.isfinite(sv)
            margin = min(margin, float((above[fin] - top_p).abs().min()))
            out[r, si[~keep]] = -float("inf")
        s = out
    return s, margin


def token_logprob(scores, tok):
    """log_softmax(scores)[tok] in float64; scores [rows, V] (-inf = removed), tok [rows]; a row of -inf gives -inf"""
    s = scores.double()
    lse = torch.logsumexp(s, -1)
    got = s.gather(1, tok.view(-1, 1).long()).squeeze(1)
    return torch.where(torch.isinf(lse) & (lse < 0), torch.full_like(lse, -float("inf")), got - lse)


def sequence_scores(logprob, seq, length, eos_id, n, length_penalty, n_out):
    """klab_gen_finalize on the host in float64: (len int [M], score float64 [M], order int [B * n_out]) from logprob [M, >= length]
    and seq [M, >= length]; len = tokens through the first EOS (length - 1 without), score = sum_{p = 1 .. len} / len ** penalty,
    order = per image of n rows the n_out best rows, equal scores in ascending row"""
    lp = np.asarray(logprob, dtype=np.float64)
    sq = np.asarray(seq)
    M = lp.shape[0]
    lens = np.empty(M, dtype=np.int64)
    score = np.empty(M, dtype=np.float64)
    for r in range(M):
        hit = np.nonzero(sq[r, 1:length] == eos_id)[0]
        lens[r] = hit[0] + 1 if len(hit) else length - 1
        score[r] = lp[r, 1:lens[r] + 1].sum() / float(lens[r]) ** length_penalty
    order = []
    for b in range(M // n):
        rows = list(range(b * n, (b + 1) * n))
        rows.sort(key=lambda r: (-score[r], r))  # (-(-inf) = inf sorts last; Python's sort is stable and the key breaks ties by row)
        order += rows[:n_out]
    return lens, score, np.asarray(order, dtype=np.int64)
