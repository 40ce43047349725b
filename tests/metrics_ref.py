"""References for the caption metrics (csrc/metrics.hip, klab_multimodalmodel_amd/metrics.py), written straight from the definitions:
the integer statistics with Counters of tuples and the textbook LCS table, the COCO caption tools' BLEU and ROUGE-L formulas with
`math`, and the fixture set of the CPU and GPU tests.  Nothing here shares code with the package."""
import math
import random
from collections import Counter
from functools import lru_cache

import torch

EOS, PAD, START = 1, 0, 0
TINY, SMALL = 1e-15, 1e-9
NAMES = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L")


# ---- the integers ----------------------------------------------------------------------------------------------------------------------
def units(seq, eos=EOS, count_eos=False):
    """the tokens through the first EOS (the EOS itself when count_eos); an id < 0 or >= 0xFFFF ends the sequence"""
    out = []
    for t in seq:
        t = int(t)
        if t < 0 or t >= 0xFFFF:
            break
        if t == eos:
            if count_eos:
                out.append(t)
            break
        out.append(t)
    return out


def grams(u, n):
    return Counter(tuple(u[i:i + n]) for i in range(len(u) - n + 1))


def lcs(a, b):
    """the textbook table: T[i][j] = LCS of a[:i] and b[:j]"""
    T = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            T[i][j] = T[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(T[i - 1][j], T[i][j - 1])
    return T[len(a)][len(b)]


def stats_row(h, present):
    """the 16 integers of one hypothesis (its units) against the PRESENT references (their units)"""
    row = [0] * 16
    if not present:
        return row
    for n in range(1, 5):
        clip = Counter()
        for rf in present:
            clip |= grams(rf, n)  # (Counter union: the maximum of the counts)
        row[n - 1] = sum((grams(h, n) & clip).values())  # (intersection: the minimum)
        row[3 + n] = max(0, len(h) - n + 1)
    row[8] = len(h)
    best = None
    for rf in present:
        if best is None or abs(len(rf) - len(h)) < abs(best - len(h)) or (abs(len(rf) - len(h)) == abs(best - len(h)) and len(rf) < best):
            best = len(rf)
    row[9] = best
    pair = (0, 0)
    for rf in present:
        l = lcs(h, rf)
        row[10] = max(row[10], l)
        if len(rf) >= 1 and (pair[1] == 0 or l * pair[1] > pair[0] * len(rf)):
            pair = (l, len(rf))
    row[11], row[12] = pair
    row[13] = len(present)
    return row


def stats(hyp, refs, n_h, eos=EOS, count_eos=False):
    """int32 [rows, 16]: stats_row of every row of hyp (int64 [rows, L], column 0 the start token) against the present rows of
    refs[row // n_h] (int64 [B, R, Lr]; a row whose first entry is negative is absent)"""
    hyp, refs = torch.as_tensor(hyp).tolist(), torch.as_tensor(refs).tolist()
    present = [[units(rf, eos, count_eos) for rf in image if rf[0] >= 0] for image in refs]
    return torch.tensor([stats_row(units(h[1:], eos, count_eos), present[r // n_h]) for r, h in enumerate(hyp)], dtype=torch.int32)


# ---- the formulas ----------------------------------------------------------------------------------------------------------------------
def bleu(match, guess, c, r):
    """[Bleu_1 .. Bleu_4] of the COCO caption tools from clipped matches, guesses, test length and reference length"""
    ratio = (c + TINY) / (r + SMALL)
    penalty = math.exp(1 - 1 / ratio) if ratio < 1 else 1.0
    out, prod = [], 1.0
    for n in range(4):
        prod *= (match[n] + TINY) / (guess[n] + SMALL)
        out.append(prod ** (1.0 / (n + 1)) * penalty)
    return out


def rouge_l(row, beta=1.2):
    if row[8] == 0 or row[12] == 0:
        return 0.0
    p, q = row[10] / row[8], row[11] / row[12]
    if p == 0 or q == 0:
        return 0.0
    return (1 + beta ** 2) * p * q / (q + beta ** 2 * p)


def sentence(row, beta=1.2):
    """[Bleu_1 .. Bleu_4, ROUGE_L] of one row of statistics; zeros without a present reference"""
    row = [int(x) for x in row]
    if row[13] == 0:
        return [0.0] * 5
    return bleu(row[0:4], row[4:8], row[8], row[9]) + [rouge_l(row, beta)]


def corpus(rows, beta=1.2):
    """the corpus numbers over rows of statistics (one per image): BLEU from the summed integers, ROUGE_L the mean, images without
    a present reference skipped"""
    rows = [[int(x) for x in r] for r in rows if int(r[13]) > 0]
    if not rows:
        return dict(zip(NAMES, [0.0] * 5), images=0)
    s = [sum(r[k] for r in rows) for k in range(10)]
    out = dict(zip(NAMES, bleu(s[0:4], s[4:8], s[8], s[9])))
    out["ROUGE_L"] = math.fsum(rouge_l(r, beta) for r in rows) / len(rows)
    out["images"] = len(rows)
    return out


# ---- the anchors of the issue: words mapped to arbitrary distinct ids ----------------------------------------------------------------
WORDS = {w: 10 + 7 * i for i, w in enumerate("the cat is on mat there a sat".split())}
ANCHOR_REFS = ["the cat is on the mat", "there is a cat on the mat"]
ANCHORS = {
    "the the the the the the the": ([2, 0, 0, 0, 7, 6, 5, 4, 7, 7, 2, 2, 6, 2], 0.2857142856326532, 1.2421889947162098e-12,
                                    0.31202046035805625),
    "a cat sat on the mat": ([5, 3, 1, 0, 6, 5, 4, 3, 6, 6, 5, 5, 7, 2], 0.8333333330555557, 8.034284186199331e-05, 0.7587064676616916),
}


def ids(sentence_):
    return [WORDS[w] for w in sentence_.split()]


# ---- the fixture set -------------------------------------------------------------------------------------------------------------------
def hyp_row(tokens, L, eos=True, junk=None):
    """a generate row of L columns: start token, the tokens, EOS (unless eos=False), then pads -- or `junk` repeated"""
    row = [START] + list(tokens) + ([EOS] if eos else [])
    assert len(row) <= L, (len(row), L)
    fill = L - len(row)
    return row + ([PAD] * fill if junk is None else (list(junk) * fill)[:fill])


def ref_row(tokens, Lr, eos=True, junk=None):
    """a label row: the tokens, EOS, -100 behind (or `junk` repeated); None = an absent reference"""
    if tokens is None:
        return [-100] * Lr
    row = list(tokens) + ([EOS] if eos else [])
    assert len(row) <= Lr, (len(row), Lr)
    fill = Lr - len(row)
    return row + ([-100] * fill if junk is None else (list(junk) * fill)[:fill])


FOUR = (2, 3, 4, 5)  # a 4-id vocabulary: repeats and clipping dominate


@lru_cache(maxsize=None)
def cases():
    """dict name -> dict(hyp int64 [rows, L], refs int64 [B, R, Lr], n_h, count_eos).  Callers must not write into it."""
    rng = random.Random(2024)
    out = {}

    def add(name, hyp, refs, n_h, count_eos=False):
        hyp, refs = torch.tensor(hyp, dtype=torch.int64), torch.tensor(refs, dtype=torch.int64)
        assert hyp.shape[0] == refs.shape[0] * n_h
        out[name] = dict(hyp=hyp, refs=refs, n_h=n_h, count_eos=count_eos)

    def draw(k, alphabet=FOUR):
        return [rng.choice(alphabet) for _ in range(k)]

    # 0, 1, 3, 4, 63 and 64 units (and 2, 5, 62: nine hypotheses, more than the waves of a workgroup) against references of 64, 3
    # and 5 units; the 64-unit hypothesis fills all 65 columns without an EOS; junk behind every EOS
    for ce in (False, True):
        long_ref = draw(64 - ce)
        refs = [[ref_row(long_ref, 64, eos=ce), ref_row(draw(3 - ce), 64, junk=FOUR), ref_row(draw(5 - ce), 64)]]
        hyps = []
        for u in (0, 1, 3, 4, 63, 64, 2, 5, 62):
            k = u - ce  # tokens in front of the EOS
            if k < 0:
                hyps.append([START, 0xFFFF] + draw(63))  # no unit even though the EOS would count: an id that ends the sequence
            elif u == 64:
                hyps.append(hyp_row(long_ref[:40] + draw(24), 65, eos=False))  # (64 units under either rule)
            else:
                body = long_ref[:k] if u in (3, 63) else draw(k)
                hyps.append(hyp_row(body, 65, junk=FOUR + (EOS,)))
        add(f"lengths count_eos={ce}", hyps, refs, 9, ce)

    # B = 7 images of n_h = 5, R = 5 over the 4-id vocabulary: absent references first, in the middle and all of them, a present
    # reference without units, an EOS first, no EOS at all, junk behind the EOS
    for ce in (False, True):
        hyps, refs = [], []
        for b in range(7):
            image = []
            for j in range(5):
                absent = b == 6 or (b == 1 and j == 0) or (b == 2 and j in (1, 3)) or (b == 3 and j != 4)
                if absent:
                    image.append(ref_row(None, 16))
                elif b == 4 and j == 1:
                    image.append([EOS] + [-100] * 15 if not ce else [0xFFFF] + draw(15))  # present, no units
                else:
                    image.append(ref_row(draw(rng.randint(1, 14)), 16, junk=FOUR if j == 2 else None))
            refs.append(image)
            hyps += [hyp_row([], 20, junk=FOUR), hyp_row(draw(19), 20, eos=False), hyp_row(units(image[4]), 20),
                     hyp_row(draw(rng.randint(1, 18)), 20, junk=FOUR + (EOS,)), hyp_row(draw(rng.randint(4, 10)), 20)]
        add(f"batch count_eos={ce}", hyps, refs, 5, ce)

    # R = 16 with the first, a middle and the last reference absent; B = 2, n_h = 1, a wider vocabulary
    wide = tuple(range(2, 12))
    refs = [[ref_row(None if j in (0, 7, 15) else draw(rng.randint(3, 14), wide), 16) for j in range(16)] for _b in range(2)]
    add("sixteen references", [hyp_row(units(refs[0][5])[:4] + units(refs[0][9])[2:], 20), hyp_row(draw(9, wide), 20)], refs, 1)
    # R = 1, B = 3: a copy of the reference, an absent reference, a disjoint hypothesis
    one = draw(9, wide)
    add("one reference", [hyp_row(one, 14), hyp_row(one, 14), hyp_row([40, 41, 42], 14)],
        [[ref_row(one, 13)], [ref_row(None, 13)], [ref_row(one, 13)]], 1)
    # B = 1, the ids 2 and 65534 (the largest an n-gram key holds)
    big = 65534
    add("extreme ids", [hyp_row([big, 2, big, big, 2, 2, big], 12), hyp_row([2, big], 12), hyp_row([big] * 11, 12, eos=False)],
        [[ref_row([big, big, 2, 2, big, big, 2], 8), ref_row([2, big, 2], 8)]], 3)
    # ties.  Image 0: the closest length, 4 against 6 for 5 units, the longer reference first -- the shorter wins.  Image 1: the recall
    # ratio, 3 / 6 first and 2 / 4 second, image 2 the same references swapped -- the lower index wins either way
    a, b_ = [20, 21, 22, 30, 31, 32], [20, 21, 40, 41]
    add("ties", [hyp_row([20, 21, 22, 50, 51], 8), hyp_row([20, 21, 22, 50, 51], 8), hyp_row([20, 21, 22, 50, 51], 8)],
        [[ref_row([60, 61, 62, 63, 64, 65], 8), ref_row([60, 61, 62, 63], 8)], [ref_row(a, 8), ref_row(b_, 8)], [ref_row(b_, 8), ref_row(a, 8)]], 1)
    return out


@lru_cache(maxsize=None)
def case_reference(name):
    """stats() of a case of cases(): int32 [rows, 16].  Callers must not write into it."""
    c = cases()[name]
    return stats(c["hyp"], c["refs"], c["n_h"], EOS, c["count_eos"])
