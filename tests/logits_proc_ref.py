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
