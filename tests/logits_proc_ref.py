"""Torch restatement of HF's logits processors as generate builds and orders them (transformers/generation/logits_process.py:
RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor, MinLengthLogitsProcessor,
MinNewTokensLengthLogitsProcessor; generation/utils.py `_get_logits_processor`) for an encoder-decoder model, whose history is
the decoder sequence with its start token (prompt length 1)."""
import torch

EOS = 1


def hf_process(hist, scores, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None, min_length=0, min_new_tokens=None,
               eos_id=EOS, log_softmax=False):
    """HF's processors as constructed (generate's own length handling: generate_processors).  hist [rows, cur_len] int64
    (position 0 = the start token), scores [rows, V] (any float dtype, widened to fp32 first as HF's `_sample` does;
    log_softmax=True: HF's `_beam_search` processes log_softmax(logits)).  Returns fp32 [rows, V]."""
    s = scores.float()
    if log_softmax:
        s = torch.log_softmax(s, -1)
    s = s.clone()
    rows, L = hist.shape
    V = s.shape[-1]
    if repetition_penalty != 1.0:
        g = torch.gather(s, 1, hist)
        g = torch.where(g < 0, g * repetition_penalty, g / repetition_penalty)
        s = s.scatter(1, hist, g)
    ban = torch.zeros(rows, V, dtype=torch.bool)
    n = no_repeat_ngram_size
    if n > 0 and L >= n:
        for r in range(rows):
            h = hist[r].tolist()
            prefix = h[L - n + 1:]
            for w in range(L - n + 1):
                if h[w:w + n - 1] == prefix:
                    ban[r, h[w + n - 1]] = True
    if bad_words_ids:
        for word in bad_words_ids:
            if word == [eos_id] or len(word) > L:
                continue
            for r in range(rows):
                if len(word) == 1 or hist[r, L - len(word) + 1:].tolist() == word[:-1]:
                    ban[r, word[-1]] = True
    if L < min_length or (min_new_tokens is not None and L - 1 < min_new_tokens):
        ban[:, eos_id] = True
    return s.masked_fill(ban, -float("inf"))


def generate_processors(kwargs):
    """the processor settings HF's generate makes of its keyword arguments: `_prepare_generated_length` replaces min_length by
    min_new_tokens + the prompt length (1, the start token) when min_new_tokens is given"""
    kw = {k: kwargs[k] for k in ("repetition_penalty", "no_repeat_ngram_size", "bad_words_ids", "min_length", "min_new_tokens") if k in kwargs}
    if kw.get("min_new_tokens") is not None:
        kw["min_length"] = kw["min_new_tokens"] + 1
    return kw


# ---- the kernel's own statement, exact in f32 (tests/test_logits_proc_exact_gpu.py) ------------------------------------------------------
def process_reference(hist, scores, V, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=(), min_length=0, min_new_tokens=0,
                      eos_id=EOS, log_softmax=False, mut=None):
    """klab_logits_process_rows as csrc/logits_proc.hip states it, in f32: hist [rows, cur_len] (position 0 = the start token; an id
    outside [0, V) marks nothing, wherever it stands), scores [rows, >= V] -> [rows, V] f32.  The penalty is one f32 multiply (score
    < 0) or divide of the original score, however often the token occurs; a ban is -inf.  log_softmax: fp64, rounded to f32, before
    both.  With log_softmax off every value is an IEEE result of the inputs: torch.equal is a fair demand.  `mut` names a wrong
    kernel (the CPU test shows the exact assertion rejects each)."""
    s = scores[:, :V].float()
    if log_softmax:
        s = torch.log_softmax(s.double(), -1).float()
    rows, L = hist.shape
    pen = torch.zeros(rows, V, dtype=torch.int32)
    ban = torch.zeros(rows, V, dtype=torch.bool)

    def mark(t):
        """the token an id marks, or None"""
        if mut == "id wrapped modulo V":
            t = t % V
        if not 0 <= t < V:
            return None
        if mut == "bit off by one":
            t = (t & ~31) | ((t + 1) & 31)
        return t if t < V else None

    n = no_repeat_ngram_size
    singles = sorted({mark(w[0]) for w in bad_words_ids if len(w) == 1} - {None})  # a one-token entry bans its token in every row
    ban[:, singles] = True
    longer = [w for w in bad_words_ids if len(w) > 1]
    for r in range(rows):
        h = hist[r].tolist()
        if repetition_penalty != 1.0:
            ids = [m for m in map(mark, h) if m is not None]
            pen[r] = torch.bincount(torch.tensor(ids, dtype=torch.int64), minlength=V).int()
        if n > 0 and L >= n:
            prefix = h[L - n + 1:]
            hits = {mark(h[w + n - 1]) for w in range(L - n + (0 if mut == "last window skipped" else 1)) if h[w:w + n - 1] == prefix}
            ban[r, sorted(hits - {None})] = True
        for word in longer:
            if len(word) <= L and h[L - len(word) + 1:] == list(word[:-1]) and mark(word[-1]) is not None:
                ban[r, mark(word[-1])] = True
        if (L < min_length or L - 1 < min_new_tokens) and 0 <= eos_id < V:
            ban[r, eos_id] = True
    p = torch.full_like(s, repetition_penalty)
    once = torch.where(s < 0, s * p, s / p)
    out = torch.where(pen > 0, once, s)
    if mut == "penalty twice":
        out = torch.where(pen > 1, torch.where(once < 0, once * p, once / p), out)
    return out.masked_fill(ban, -float("inf"))


PROC_VOCABS = (5, 33, 1000, 1057, 32768)
PROC_CUR = (1, 2, 3, 64, 1024)
PROC_ROWS = 4  # logits rows; times row_div history rows


def forced_tokens(V):
    """the ids every long enough history holds: 0, 31 and 32 (the edge between bitmap words 0 and 1), V-1, and a token of the last
    word of the bitmap, which is partial when V % 32 != 0"""
    return [0, min(31, V - 1), min(32, V - 1), V - 1, max(0, ((V - 1) // 32) * 32 + ((V - 1) % 32) // 2)]


def proc_fixture(V, row_div, cur):
    """(x [PROC_ROWS, V] fp64 on a 0.25 grid in [-8, 8], exact in bf16; hist [PROC_ROWS*row_div, cur] int64).  Row 0 holds an exact
    tie at the maximum (9.0) between two tokens of different waves where the vocabulary has two waves (one wave: 2048 tokens), of
    different threads otherwise.  Histories draw from the whole vocabulary, with the forced tokens rotated in from position 1, a
    repeated token, one id >= V and one negative id (cur >= 3); the last history row draws from three tokens only, so that many
    n-gram windows match at once."""
    g = torch.Generator().manual_seed(31 * V + 7 * row_div + cur)
    x = torch.randint(-32, 33, (PROC_ROWS, V), generator=g).double() * 0.25
    x[0, tie_tokens(V)] = 9.0
    rows = PROC_ROWS * row_div
    hist = torch.randint(0, V, (rows, cur), generator=g)
    F = forced_tokens(V)
    for r in range(rows):
        for p in range(1, min(cur, len(F) + 1)):
            hist[r, p] = F[(r + p) % len(F)]
        if cur >= 12:
            hist[r, 8:12] = hist[r, 7]  # repeats
    if cur >= 3:
        hist[1, 1] = V + 3
        hist[2, 2] = -2
        hist[0, 2] = hist[0, 1]
    if cur >= 8:
        hist[rows - 1] = torch.tensor([F[0], F[3], F[4]])[torch.randint(0, 3, (cur,), generator=g)]
    hist[:, 0] = 0
    return x, hist


def tie_tokens(V):
    return [100, 5000] if V > 2048 else [min(1, V - 2), V - 1]


def proc_settings(V):
    """the existing SETTINGS with their tokens taken from the forced set, a bad-word list long enough for the kernel's entry loop to
    lap (1100 single tokens spread over the vocabulary, EOS left out), and the n-gram sizes that find several windows in the
    three-token history"""
    a, b, c, d, e = forced_tokens(V)
    spread = [t for t in ((i * max(1, V // 1100) + 3 * (i % 7)) % V for i in range(2000)) if t != EOS][:1100]
    return [
        dict(repetition_penalty=1.3),
        dict(repetition_penalty=0.6, no_repeat_ngram_size=2),
        dict(no_repeat_ngram_size=1, min_length=9),
        dict(bad_words_ids=[[b], [c, d], [e, e, e], [a] * 20]),
        dict(repetition_penalty=1.2, no_repeat_ngram_size=3, bad_words_ids=[[a, b, c], [d, e], [a, d]], min_length=4, min_new_tokens=6),
        dict(bad_words_ids=[[t] for t in spread]),
        dict(no_repeat_ngram_size=2, repetition_penalty=1.5),
    ]
