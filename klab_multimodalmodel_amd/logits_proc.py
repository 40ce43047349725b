"""Argument handling of MyModel.generate's logits processors, as HF's `generate` does it for an encoder-decoder model
(transformers 5.15: `_prepare_generated_length` and `_get_logits_processor` in generation/utils.py, the processors' constructors
and first call in generation/logits_process.py).  Pure Python: no GPU, no engine."""
import numpy as np

MAX_BAD_WORD_TOKENS = 1024  # the device table's cap (csrc/logits_proc.hip)


def logits_processor_settings(repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None, min_length=0, min_new_tokens=None,
                              *, eos_token_id, vocab_size, prompt_length=1):
    """HF's checks, in HF's order and with HF's exception types and messages.  prompt_length is HF's decoder prompt length, the
    start token counted: 1 without generate(decoder_input_ids=...).  `min_new_tokens` (when given) replaces `min_length` by
    min_new_tokens + prompt_length, whatever min_length was, and the kernel's own min_new_tokens test, which counts generated
    tokens from position 1 (cur_len - 1 < min_new_tokens), is given min_new_tokens + prompt_length - 1.  Returns None when no processor would change a score, else the settings the engine runs:
    dict(repetition_penalty, no_repeat_ngram_size, bad_words_ids (entries equal to [eos] dropped), min_length, min_new_tokens)."""
    if min_new_tokens is not None:
        min_length = min_new_tokens + prompt_length
    out = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=[], min_length=0, min_new_tokens=0)
    # RepetitionPenaltyLogitsProcessor
    if repetition_penalty is not None and repetition_penalty != 1.0:
        if not isinstance(repetition_penalty, float) or not (repetition_penalty > 0):
            raise ValueError(f"`penalty` has to be a strictly positive float, but is {repetition_penalty}")
        out["repetition_penalty"] = float(repetition_penalty)
    # NoRepeatNGramLogitsProcessor
    if no_repeat_ngram_size is not None and no_repeat_ngram_size > 0:
        if not isinstance(no_repeat_ngram_size, int) or no_repeat_ngram_size <= 0:
            raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {no_repeat_ngram_size}")
        out["no_repeat_ngram_size"] = int(no_repeat_ngram_size)
    # NoBadWordsLogitsProcessor -> SequenceBiasLogitsProcessor with bias -inf
    bias = None
    if bad_words_ids is not None:
        if not isinstance(bad_words_ids, list) or len(bad_words_ids) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad_words_ids}.")
        if any(not isinstance(bad_word_ids, list) for bad_word_ids in bad_words_ids):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bad_words_ids}.")
        if any(any((not isinstance(t, (int, np.integer)) or t < 0) for t in bad_word_ids) for bad_word_ids in bad_words_ids):
            raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bad_words_ids}.")
        # ([eos] entries dropped; the base class's own checks never run, NoBadWords overrides them)
        bias = {tuple(w): float("-inf") for w in bad_words_ids if w != [eos_token_id]}
    # MinLengthLogitsProcessor
    if min_length is not None and min_length > 0:
        if not isinstance(min_length, int) or min_length < 0:
            raise ValueError(f"`min_length` has to be a non-negative integer, but is {min_length}")
        out["min_length"] = int(min_length)
    # MinNewTokensLengthLogitsProcessor (prompt_length_to_skip = prompt_length)
    if min_new_tokens is not None and min_new_tokens > 0:
        if not isinstance(min_new_tokens, int) or min_new_tokens < 0:
            raise ValueError(f"`min_new_tokens` has to be a positive integer, but is {min_new_tokens}")
        out["min_new_tokens"] = int(min_new_tokens) + prompt_length - 1
    # SequenceBiasLogitsProcessor._prepare_bias_variables (HF's first call)
    if bias is not None:
        invalid = [t for ids in bias for t in ids if t >= vocab_size]
        if invalid:
            raise ValueError(f"The model vocabulary size is {vocab_size}, but the following tokens were being biased: {invalid}")
        if any(len(ids) == 0 for ids in bias):
            raise IndexError("tuple index out of range")  # what HF's first call raises on an empty entry (`sequence_ids[-1]`)
        out["bad_words_ids"] = [[int(t) for t in ids] for ids in bias]
        n_tok = sum(len(w) for w in out["bad_words_ids"])
        if n_tok > MAX_BAD_WORD_TOKENS:
            raise NotImplementedError(f"bad_words_ids: at most {MAX_BAD_WORD_TOKENS} tokens in all are supported, got {n_tok}")
    active = (out["repetition_penalty"] != 1.0 or out["no_repeat_ngram_size"] > 0 or out["bad_words_ids"] or out["min_length"] > 1
              or out["min_new_tokens"] > 0)  # (min_length 1 bans nothing: cur_len counts the start token)
    return out if active else None
