"""References for self-critical training (csrc/scst.hip, klab_multimodalmodel_amd/scst.py), written straight from the definitions:
CIDEr-D over token ids with Counters of tuples (fp64, or every operation rounded to fp32), the numpy statement of the idf table's
probe, the targets kernel, and the fixture set of the GPU reward test with the tolerance derived from it."""
import math
import random
from collections import Counter
from functools import lru_cache

import numpy as np
import torch

EOS, PAD, START = 1, 0, 0
EMPTY = 0xFFFFFFFFFFFFFFFF
GOLDEN = 0x9E3779B97F4A7C15

# The reward tolerance: 8x the largest |fp32 mode - fp64 mode| of reward() over reward_cases(), the GPU test's fixture set
# (tests/test_scst_cpu.py recomputes it).  The factor covers the kernel's other summation order (wave trees) and the hardware's
# exp / sqrt / divide.  Rewards reach 10; an fp32 emulation on 2000 random cases gave 1.2e-6 -- orientation, not the bound.
REWARD_TOL_FACTOR = 8.0
REWARD_TOL = 4.168764348833065e-06


# ---- units, n-grams, document frequency ---------------------------------------------------------------------------------------------
def units(seq, eos=EOS, count_eos=True):
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


def doc_freq(corpus, eos=EOS, count_eos=True):
    """{n-gram: number of IMAGES one of whose references holds it}; corpus: per image a list of id lists"""
    df = Counter()
    for image in corpus:
        seen = set()
        for cap in image:
            u = units(cap, eos, count_eos)
            for n in range(1, 5):
                seen.update(grams(u, n))
        df.update(seen)
    return df


def idf64(g, df, n_images):
    return math.log(n_images) - math.log(max(1, df.get(g, 0)))


def reward(hyp_units, ref_units, df, n_images, sigma=6.0, fp32=False):
    """CIDEr-D of one hypothesis (its units) against the PRESENT references (their units).  fp32: idf rounded once and every
    operation after it rounded to fp32 (numpy float32 scalars stay float32)."""
    T = np.float32 if fp32 else np.float64
    if not ref_units or not hyp_units:
        return T(0.0)

    def vec(u, n):
        v = {g: T(c) * T(idf64(g, df, n_images)) for g, c in grams(u, n).items()}
        s = T(0.0)
        for x in v.values():
            s = s + x * x
        return v, np.sqrt(s)

    total = T(0.0)
    for n in range(1, 5):
        vh, nh = vec(hyp_units, n)
        score = T(0.0)
        for ru in ref_units:
            vr, nr = vec(ru, n)
            sim = T(0.0)
            for g, x in vh.items():
                y = vr.get(g, T(0.0))
                sim = sim + min(x, y) * y
            if nh != 0 and nr != 0:
                sim = sim / (nh * nr)
            d = T(len(hyp_units) - len(ru))
            sim = sim * T(math.exp(-(d * d) / (T(2.0) * T(sigma) * T(sigma))))  # (exp in fp64, rounded once: the same on every host)
            score = score + sim
        total = total + score / T(len(ref_units))
    return T(10.0) * (total / T(4.0))


def rewards(hyp, refs, n_h, df, n_images, eos=EOS, count_eos=True, sigma=6.0, fp32=False):
    """[rows] float64 array: reward() of every row of hyp (int64 [rows, L], column 0 the start token) against the present rows of
    refs[row // n_h] (int64 [B, R, Lr]; a row whose first entry is negative is absent)"""
    hyp, refs = np.asarray(hyp), np.asarray(refs)
    out = np.zeros(hyp.shape[0])
    for r in range(hyp.shape[0]):
        ru = [units(row, eos, count_eos) for row in refs[r // n_h] if row[0] >= 0]
        out[r] = float(reward(units(hyp[r, 1:], eos, count_eos), ru, df, n_images, sigma, fp32))
    return out


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def gram_key(g):
    """t0 | t1 << 16 | t2 << 32 | t3 << 48, absent positions 0xFFFF"""
    k = 0
    for i in range(4):
        k |= (int(g[i]) if i < len(g) else 0xFFFF) << (16 * i)
    return k


def home_slot(key, cap):
    return ((key * GOLDEN) & EMPTY) >> (64 - (cap.bit_length() - 1))


def table_lookup(keys, idf, key, log_n):
    """the probe as the kernel runs it: (value, slot or -1, probes).  keys: numpy uint64 [cap], idf: float32 [cap]"""
    cap = len(keys)
    slot = home_slot(key, cap)
    for p in range(cap):
        k = int(keys[slot])
        if k == key:
            return float(idf[slot]), slot, p + 1
        if k == EMPTY:
            break
        slot = (slot + 1) & (cap - 1)
    return float(log_n), -1, 0


# ---- klab_scst_targets ---------------------------------------------------------------------------------------------------------------
def targets(seq, rew, baseline, mode, n, Lt, eos=EOS):
    """(labels int64 [rows, Lt], weights fp32 [rows, Lt], advantages fp32 [rows]); fp32 arithmetic in the kernel's order"""
    seq = torch.as_tensor(seq)
    rows, L = seq.shape
    rew = np.asarray(torch.as_tensor(rew), dtype=np.float32)
    labels = torch.full((rows, Lt), -100, dtype=torch.int64)
    weights = torch.zeros(rows, Lt, dtype=torch.float32)
    adv = torch.zeros(rows, dtype=torch.float32)
    for r in range(rows):
        b = r // n
        a = rew[r]
        if mode == 0:
            a = a - np.float32(baseline[b])
        elif mode == 1:
            others = np.float32(0.0)
            for k in range(b * n, (b + 1) * n):
                if k != r:
                    others = others + rew[k]
            a = a - others / np.float32(n - 1)
        row = seq[r, 1:].tolist()
        last = row.index(eos) if eos in row else L - 2
        for t in range(last + 1):
            labels[r, t] = row[t]
            weights[r, t] = float(a)
        adv[r] = float(a)
    return labels, weights, adv


# ---- the GPU reward test's fixture set ---------------------------------------------------------------------------------------------
def _caption(rng, lo, hi, alphabet):
    return [rng.choice(alphabet) for _ in range(rng.randint(lo, hi))] + [EOS]


def corpus(seed=0, images=12, per_image=5, alphabet=tuple(range(2, 13))):
    """per image a list of EOS-closed id lists over a small alphabet, so that n-grams repeat within and across images"""
    rng = random.Random(seed)
    return [[_caption(rng, 2, 12, alphabet) for _ in range(per_image)] for _ in range(images)]


def hyp_row(tokens, L, eos=True):
    """a generate row of L columns: start token, the tokens, EOS (unless eos=False), pads"""
    row = [START] + list(tokens) + ([EOS] if eos else [])
    assert len(row) <= L, (len(row), L)
    return row + [PAD] * (L - len(row))


def ref_row(tokens, Lr, eos=True):
    """a label row: the tokens, EOS, -100 behind; None = an absent reference"""
    if tokens is None:
        return [-100] * Lr
    row = list(tokens) + ([EOS] if eos else [])
    assert len(row) <= Lr
    return row + [-100] * (Lr - len(row))


WRAP_SEED = 28  # corpus(WRAP_SEED) at its smallest capacity holds a probe chain that wraps around the end (test_scst_cpu.py)


@lru_cache(maxsize=None)
def reward_cases():
    """dict name -> dict(corpus, V, count_eos, capacity, hyp [rows, L], refs [B, R, Lr], n_h).  Callers must not write into it."""
    rng = random.Random(77)
    small = tuple(range(2, 13))
    cases = {}

    def add(name, hyp, refs, n_h, corp=None, V=64, count_eos=True, capacity=None):
        cases[name] = dict(corpus=corpus() if corp is None else corp, V=V, count_eos=count_eos, capacity=capacity,
                           hyp=torch.tensor(hyp, dtype=torch.int64), refs=torch.tensor(refs, dtype=torch.int64), n_h=n_h)

    # 1, 3, 4, 63 and 64 units against a 64-unit and a 4-unit reference: empty higher orders and the wave boundary; a small alphabet repeats
    # tokens, so counts exceed 1 and the min clips
    # (20 and 21 are in no reference of the corpus: their n-grams weigh log_n; the short second reference keeps the length
    # penalty from wiping out the short hypotheses)
    long_ref = [rng.choice((2, 3, 20, 21)) for _ in range(63)]
    for ce in (True, False):
        hyps = [hyp_row([], 65), hyp_row(long_ref[:2], 65), hyp_row(long_ref[:3], 65), hyp_row(long_ref[:62], 65),
                hyp_row(long_ref[:63], 65)] if ce else \
               [hyp_row(long_ref[:1], 65), hyp_row(long_ref[:3], 65), hyp_row(long_ref[:4], 65), hyp_row(long_ref[:63], 65),
                hyp_row(long_ref[:63] + [5], 65, eos=False)]
        ref = ref_row(long_ref, 64) if ce else ref_row(long_ref + [7], 64, eos=False)
        add(f"lengths count_eos={ce}", hyps, [[ref, ref_row(long_ref[:3], 64)]], 5, count_eos=ce)
    # B = 3, n_h = 5, R = 5 with absent references; the last image has none.  EOS first, no EOS, a copy of a reference, repeats
    corp = corpus()
    for ce in (True, False):
        hyps, refs = [], []
        for b in range(3):
            caps = [c[:-1] for c in corp[b]]
            refs.append([ref_row(None if b == 2 or (b == 1 and j in (0, 3)) else caps[j], 16) for j in range(5)])
            hyps += [hyp_row([], 20), hyp_row([rng.choice(small) for _ in range(19)], 20, eos=False), hyp_row(caps[1], 20),
                     hyp_row(caps[2][:3] + caps[2][:3] + caps[4][:2], 20), hyp_row([rng.choice(small) for _ in range(7)], 20)]
        add(f"batch count_eos={ce}", hyps, refs, 5, count_eos=ce)
        if ce:
            add("batch wrapped table", hyps, refs, 5, corp=corpus(WRAP_SEED), capacity="smallest")
    # R = 16 with some absent, R = 1, n_h = 1
    caps = [c[:-1] for im in corp[3:7] for c in im][:16]
    add("sixteen references", [hyp_row(caps[5][:4] + caps[9][2:], 20)],
        [[ref_row(None if j in (0, 7, 15) else caps[j], 16) for j in range(16)]], 1)
    add("one reference", [hyp_row(corp[0][0][:-1], 14), hyp_row(corp[1][0][:-1], 14)],
        [[ref_row(corp[0][0][:-1], 13)], [ref_row(corp[1][1][:-1], 13)]], 1)
    # ids 0 and V - 1 of the largest vocabulary, n-grams the table does not hold (40, 41 are in no reference of the corpus)
    V = 65535
    big = [[[0, V - 1, 5, 0, EOS], [V - 1, V - 1, 6, EOS]], [[7, 0, 0, 8, EOS]], [[5, 6, 7, 8, 9, EOS]]]
    add("extreme ids", [hyp_row([0, V - 1, 5, 0], 12), hyp_row([V - 1, 40, 41, 0, 0], 12), hyp_row([40, 41, 40, 41], 12)],
        [[ref_row([0, V - 1, 5, 0], 8), ref_row([V - 1, V - 1, 6], 8), ref_row([40, 41, 5], 8)]] * 3, 1, corp=big, V=V)
    return cases


def case_reference(c, fp32=False):
    """rewards() of a case of reward_cases()"""
    df = doc_freq(c["corpus"], EOS, c["count_eos"])
    return rewards(c["hyp"], c["refs"], c["n_h"], df, len(c["corpus"]), EOS, c["count_eos"], 6.0, fp32)


def smallest_capacity(entries):
    return max(2, 1 << max(0, 2 * entries - 1).bit_length())
