"""References and fixtures for tests/test_beam_exact_gpu.py (csrc/beam.hip), plain torch on the host;
tests/test_decode_select_fixtures_cpu.py proves what the GPU test takes for granted about them.

Order.  Everything beam.hip selects is ranked by its `beam_better`: the larger score, and among equal scores the lower index -- the
flat index beam*V + token in both stages of the top-k, the position among the 2k candidates for the running beams, the position
in the [pool, candidates] concatenation for the finished pool.  The references state that as a stable descending sort of a list
that is already in index order (never torch.topk, whose tie order is unspecified), so ties are part of what is compared.

Exactness.  The `klab_beam_topk_scores` fixtures keep every score and running score on a 2^-4 grid of small magnitude: the one
f32 add of the kernel is exact, equal sums are equal bit for bit, and torch.equal on scores and indices is a fair demand.  The
first-step running scores 0 / -1e9 swallow the grid value (-1e9 + x == -1e9 in f32 for |x| < 32): every candidate of such a beam
ties and only the index rule orders them.  The log-softmax fixtures of `klab_beam_topk` plant 2k winners whose final scores lie
0.25 apart (the running score of a row carries the row's own log-sum-exp, so the final score is a grid value up to f32 rounding)
or are equal by construction: equal logits inside one row, or bit-identical rows under equal running scores.

`update_reference` is HF's `_beam_search` iteration (transformers/generation/utils.py: `_get_running_beams_for_next_iteration`,
`_update_finished_beams`, `_check_early_stop_heuristic`, `_beam_search_has_unfinished_sequences`) from the 2k candidates on, for
cur_len = c and decoder_prompt_len = 1.  `search_reference` chains it with `topk_reference` over scripted scores, with the engine's
ping-pong of the sequence and key-slot buffers (beam_args in csrc/engine.cpp: step c reads parity c+1 and writes parity c).

The `mut=` arguments produce the wrong answers of a subtly wrong kernel; the CPU test shows the exact assertions reject each."""
import functools

import torch

NEG = -1.0e9
INT_MAX = 2 ** 31 - 1
B = 3
KS = (1, 2, 3, 5, 8, 9, 12, 16)
LAYOUTS = ("dense", "odd")  # ld = V from an aligned base; ld = V + 3 from a base one element past an aligned address
EOS = 1


def kmax(k):
    """the list length beam_topk_rows_kernel is instantiated with for k beams"""
    return next(n for n in (2, 4, 8, 16, 32) if 2 * k <= n)


def threads(k):
    return 128 if kmax(k) == 32 else 256


def vocabs(k):
    return sorted({2 * k, 2 * k + 1, 1001, 4100, 4104} | ({37} if 37 >= 2 * k else set()))


def layout(name, V):
    """(ld, element offset of row 0 from a 16-byte aligned base)"""
    return (V, 0) if name == "dense" else (V + 3, 1)


def load_path(esize, V, ld, off, row):
    """which load loop beam_topk_rows_kernel takes for logits row `row`: 16-byte vectors need V % VEC == 0 and an aligned row start"""
    vec = 16 // esize
    return "vector" if V % vec == 0 and ((off + row * ld) * esize) % 16 == 0 else "scalar"


def owned_tokens(tid, V, nthreads, vec):
    """the tokens thread tid streams: vec consecutive tokens per lap on the vector path, one per lap (vec = 0) on the scalar path"""
    if not vec:
        return list(range(tid, V, nthreads))
    return [j + c for j in range(tid * vec, V, nthreads * vec) for c in range(vec)]


def device_layout(x, ld, off, gap):
    """a flat buffer holding the rows of x at off + r*ld, `gap` everywhere else (a read past V then wins and is seen), and its
    [R, ld] view; the view's first element is the pointer the kernel gets"""
    R, V = x.shape
    buf = torch.full((off + R * ld + 8,), gap, dtype=x.dtype)
    view = buf[off:off + R * ld].view(R, ld)
    view[:, :V] = x
    return buf, view


def _best(score, n, tie_high=False):
    """positions of the n best of a list in index order: score descending, equal scores by the lower position (tie_high: the
    higher one, a mutation)"""
    if tie_high:
        return score.numel() - 1 - torch.sort(score.flip(0), descending=True, stable=True)[1][:n]
    return torch.sort(score, descending=True, stable=True)[1][:n]


def _pad(s, i, n):
    if s.numel() >= n:
        return s, i
    m = n - s.numel()
    return torch.cat((s, torch.full((m,), -float("inf")))), torch.cat((i, torch.full((m,), INT_MAX, dtype=torch.int64)))


def topk_reference(scores_f32, run_score, k, V, row_div=1, normed=True, mut=None):
    """the 2k best (score, beam*V + token) of every sample: [B, 2k] f32 and [B, 2k] int64, score descending then flat index
    ascending.  scores_f32 [B*k / row_div, >= V] (the columns past V are the layout's gap and are not read), run_score [B, k].
    normed: score = row[j] + run_score[r], one f32 add; else fp64 log_softmax of the row rounded to f32, then the f32 add.
    Two stages as the kernel has them (per row, then the merge of a sample's rows), so that either can be mutated."""
    rs = run_score.reshape(-1).float()
    Bn, K2 = rs.numel() // k, 2 * k
    out_s, out_i = torch.empty(Bn, K2), torch.empty(Bn, K2, dtype=torch.int64)
    for b in range(Bn):
        ls, li = [], []
        for beam in range(k):
            r = b * k + beam
            row = scores_f32[r % scores_f32.shape[0] if mut == "row_div ignored" else r // row_div]
            hi = V - 1 if mut == "last token dropped" else V + 1 if mut == "token V read" else V
            x = row[:hi].float()
            s = (x if normed else torch.log_softmax(x.double(), -1).float()) + rs[r]
            p = _best(x if mut == "row ranked before the add" else s, K2 - 1 if mut == "list truncated" else K2, tie_high=mut == "row tie high")
            flat = (r // k if mut == "beam = r / k" else beam) * V + p
            if mut == "sentinel leak":
                flat = torch.where(s[p] == -float("inf"), torch.full_like(flat, INT_MAX), flat)
            s, flat = _pad(s[p], flat, K2)
            ls.append(s)
            li.append(flat)
        s, i = torch.cat(ls), torch.cat(li)
        o = torch.argsort(i, stable=True)
        s, i = s[o], i[o]
        p = _best(s, K2, tie_high=mut == "merge tie high")
        out_s[b], out_i[b] = s[p], i[p]
    return out_s, out_i


# ---- fixtures of klab_beam_topk_scores ---------------------------------------------------------------------------------------------
SCORE_KINDS = ("a", "a1", "b", "b2", "c", "d", "e", "e1", "f", "f1")


def _grid(g, lo16, hi16, *shape):
    """-n/16 for n drawn from lo16 .. hi16"""
    return -torch.randint(lo16, hi16 + 1, shape, generator=g).float() / 16


def first_step_scores(k):
    rs = torch.full((B, k), NEG)
    rs[:, 0] = 0.0
    return rs


@functools.lru_cache(maxsize=None)
def scores_fixture(kind, k, V, lay="dense"):
    """(x [B*k, V] f32 on the 2^-4 grid in [-16, 0] or -inf, run_score [B, k]) for the fixture table of the issue:
    a  random grid values (256 distinct values: ties everywhere);      a1 the same under the first-step 0 / -1e9 running scores
    b  the 2k winners of a sample in one beam row;                     b2 ... and among the tokens one thread streams
    c  winners at tokens 0 and V-1 of beams 0 and k-1;                 d  one winner per beam row
    e  every row holds fewer than 2k finite scores;                    e1 the same under the first-step running scores
    f  one beam row entirely -inf;                                     f1 beam 0 entirely -inf under the first-step scores
    Cached: callers must not write into what they get."""
    g = torch.Generator().manual_seed(1000 * k + V + 7 * SCORE_KINDS.index(kind))
    K2, R = 2 * k, B * k
    ld, off = layout(lay, V)
    rs = first_step_scores(k) if kind in ("a1", "e1", "f1") else _grid(g, 0, 32, B, k)
    if kind in ("a", "a1", "f", "f1"):
        x = _grid(g, 0, 256, R, V)
        for b in range(B):
            if kind in ("f", "f1"):
                x[b * k + (0 if kind == "f1" else b % k)] = -float("inf")
            else:
                x[b * k + k - 1] = x[b * k]  # beams 0 and k-1 read bit-identical rows
        return x, rs
    if kind in ("e", "e1"):
        x = torch.full((R, V), -float("inf"))
        for r in range(R):
            m = int(torch.randint(0, K2, (1,), generator=g))
            pos = torch.randperm(V, generator=g)[:m]
            x[r, pos] = _grid(g, 0, 256, m)
        return x, rs
    x = _grid(g, 128, 256, R, V)  # background in [-16, -8]; winners in [-2, 0] and running scores in [-2, 0] keep them apart
    for b in range(B):
        w = -torch.randperm(K2, generator=g).float() / 16
        if kind in ("b", "b2"):
            r = b * k + (b + 1) % k
            pos = torch.randperm(V, generator=g)[:K2].tolist()
            if kind == "b2":
                nt = threads(k)
                vec = 4 if load_path(4, V, ld, off, r) == "vector" else 0
                own = owned_tokens((5 + b) % min(nt, V // max(vec, 1)), V, nt, vec)[:K2]
                pos = own + [p for p in pos if p not in own][:K2 - len(own)]
            x[r, pos] = w
        elif kind == "c":
            spots = list(dict.fromkeys([(0, 0), (0, V - 1), (k - 1, 0), (k - 1, V - 1)]))
            for n, (beam, tok) in enumerate(spots):
                x[b * k + beam, tok] = -n / 16
        else:
            for beam in range(k):
                x[b * k + beam, int(torch.randint(0, V, (1,), generator=g))] = w[beam]
    return x, rs


# ---- fixtures of klab_beam_topk (log-softmax form) -----------------------------------------------------------------------------------
LOGIT_KINDS = ("b", "b2", "c", "d")


def _spots(kind, k, V, b, g, esize, lay, row_div):
    """2k distinct (beam, token) places of sample b's winners; the first two share a row (row_div == k: the beam is ignored)"""
    K2 = 2 * k
    ld, off = layout(lay, V)
    one_row = kind in ("b", "b2") or row_div > 1
    beam0 = (b + 1) % k if one_row else 0
    if kind == "b2":
        vec = 16 // esize if load_path(esize, V, ld, off, (b * k + beam0) // row_div) == "vector" else 0
        nt = threads(k)
        out = [(beam0, t) for t in owned_tokens((5 + b) % min(nt, V // max(vec, 1)), V, nt, vec)[:K2]]
    elif kind == "c":
        out = [(beam0, 0), (beam0, V - 1)] + ([] if one_row or k == 1 else [(k - 1, 0), (k - 1, V - 1)])
    else:
        out = []
    want = [beam0, beam0] + ([beam0] * K2 if one_row else list(range(1, k)) + [n % k for n in range(K2)])
    for beam in want[len(out):]:
        if len(out) == K2:
            break
        t = int(torch.randint(0, V, (1,), generator=g))
        while (beam, t) in out:
            t = (t + 1) % V
        out.append((beam, t))
    return out[:K2]


@functools.lru_cache(maxsize=None)
def logits_fixture(kind, k, V, row_div, dn, lay="dense", tie_rows=False):
    """(x [B*k/row_div, V] fp64 on a 0.25 grid, exact in bf16; run_score [B, k] f32).  Background in [-24, -8]; 2k winners per
    sample whose final scores are 8 - 0.25 i (the first two equal: equal logits inside one row).  run_score[r] = g[beam] + the
    row's log-sum-exp, so the final score of (beam, token) is x + g[beam] up to f32 rounding: row_div = 1 spreads the winners
    over the beams with g on the 0.25 grid; row_div = k shares one row per sample, g = -8 per rank so one beam wins all 2k, and
    tie_rows gives two beams the same running score (bit-identical rows: every winner then ties across the two beams)."""
    esize = 2 if dn == "bf16" else 4
    g = torch.Generator().manual_seed(2000 * k + V + 11 * LOGIT_KINDS.index(kind) + row_div)
    K2, R = 2 * k, B * k // row_div
    x = -(8.0 + 0.25 * torch.randint(0, 65, (R, V), generator=g).double())
    gb = torch.zeros(B, k, dtype=torch.float64)
    F = [0.0, 0.0] + [-0.25 * i for i in range(2, K2)]
    for b in range(B):
        spots = _spots(kind, k, V, b, g, esize, lay, row_div)
        if row_div == 1:
            gb[b] = -0.25 * torch.randperm(k, generator=g).double()
            for n, (beam, tok) in enumerate(spots):
                x[b * k + beam, tok] = 8.0 + F[n] - float(gb[b, beam])
        else:
            rank = torch.randperm(k, generator=g).double()
            if tie_rows and k >= 2:
                rank[rank == 1] = 0
            gb[b] = -8.0 * rank
            for n, (_beam, tok) in enumerate(spots):
                x[b, tok] = 8.0 + F[n]
    lse = torch.logsumexp(x, -1).repeat_interleave(row_div).view(B, k)
    return x, (gb + lse).float()


# ---- klab_beam_update ---------------------------------------------------------------------------------------------------------------
def _gather(t, idx):
    while idx.dim() < t.dim():
        idx = idx.unsqueeze(-1)
    return torch.take_along_dim(t, idx, dim=1)


def _order(x, n):
    """the n best of every row of x: value descending, equal values by the lower position"""
    return torch.sort(x, dim=1, descending=True, stable=True)[1][:, :n]


def _div(x, d):
    """the f32 divide of every element by float(d) (a tensor divisor: a true IEEE division)"""
    return x / torch.full_like(x, float(d))


def update_reference(st, cand_score, cand_idx, c, cfg, mut=None):
    """one iteration of `_beam_search` from the top-k candidates on (cur_len = c, decoder_prompt_len = 1).  st: run_seq / fin_seq
    [B, k, Lm] int64, fin_flag [B, k] bool, fin_score [B, k] f32, fin_len [B, k] int32, unsat [B, 1] bool; cfg: k, V, Lm, eos,
    lp (length penalty), es (early_stopping: 0 False, 1 True, 2 "never")."""
    k, V, Lm, eos, lp, es = (cfg[n] for n in ("k", "V", "Lm", "eos", "lp", "es"))
    K2 = 2 * k
    cs = cand_score
    beam, tok = cand_idx // V, cand_idx % V
    trs = _gather(st["run_seq"], beam).clone()
    trs[:, :, c] = tok
    hits = (tok == eos) | (c + 1 >= Lm)
    trl = cs + hits.float() * NEG                                                      # _get_running_beams_for_next_iteration
    ni = _order(trl, k)
    out = dict(run_seq=_gather(trs, ni), run_score=_gather(trl, ni), tok=_gather(tok, ni), par=_gather(beam, ni))
    did = hits & (torch.arange(K2) < k)[None]                                          # _update_finished_beams
    tlp = _div(cs, c ** lp)
    tlp = tlp + (st["fin_flag"].all(-1, keepdim=True) & (es == 1)).float() * NEG
    tlp = tlp + (~st["unsat"]).float() * NEG
    tlp = tlp + (~did).float() * NEG
    msc = torch.cat((st["fin_score"], tlp), 1)
    if mut == "pool tie to candidate":
        mi = (_order(torch.cat((tlp, st["fin_score"]), 1), k) + k) % (3 * k)
    else:
        mi = _order(msc, k)
    out["fin_score"] = _gather(msc, mi)
    out["fin_flag"] = _gather(torch.cat((st["fin_flag"], did), 1), mi)
    out["fin_seq"] = _gather(torch.cat((st["fin_seq"], trs), 1), mi)
    new_len = torch.full((cs.shape[0], K2), c, dtype=torch.int32)
    out["fin_len"] = _gather(torch.cat((st["fin_len"], st["fin_len"].repeat(1, 2) if mut == "fin_len kept" else new_len), 1), mi)
    bhl = (Lm - 1) if (es == 2 and lp > 0.0) else c                                    # _check_early_stop_heuristic (cur_len c+1)
    best = _div(out["run_score"][:, :1], bhl ** lp)
    worst = torch.where(out["fin_flag"], out["fin_score"].min(1, keepdim=True)[0], torch.tensor(NEG))
    out["unsat"] = st["unsat"] & (best > worst).any(-1, keepdim=True)
    out["word"] = (int(out["unsat"].any()) | (2 * int((~out["fin_flag"].all(-1)).any())) | (4 * int((~hits.all(-1)).any())))
    return out


def going(word, es):
    """does the search go on after a step with this stop word (engine.gen_going)"""
    return bool((word & 1) and (word & 4) and (es != 1 or (word & 2)))


def init_reference(Bn, k, Lm, start, fill):
    """the state klab_beam_init leaves (the slot table's columns past 0 are not written: -1 here, whatever was there on the device)"""
    seq = torch.full((Bn, k, Lm), fill, dtype=torch.int64)
    seq[:, :, 0] = start
    run_score = torch.full((Bn, k), NEG)
    run_score[:, 0] = 0.0
    slot = torch.full((Bn * k, Lm), -1, dtype=torch.int32)
    slot[:, 0] = torch.arange(Bn * k, dtype=torch.int32)
    return dict(run_seq=seq, fin_seq=seq.clone(), run_score=run_score, fin_score=torch.full((Bn, k), NEG),
                fin_flag=torch.zeros(Bn, k, dtype=torch.bool), fin_len=torch.zeros(Bn, k, dtype=torch.int32),
                unsat=torch.ones(Bn, 1, dtype=torch.bool), slot=slot, stop=torch.zeros(Lm, dtype=torch.int32))


START, FILL = 0, 7


def search_reference(score_fn, Bn, k, V, Lm, cfg, mut=None):
    """init_reference, then topk_reference(normed) and update_reference for c = 1 .. Lm-1 with the in / out buffers swapped by the
    parity of c, until the stop word ends the search.  Returns the list of states, [0] = after init, [c] = after step c: every
    field of update_reference's result plus cand_score / cand_idx, rows (the parent row of every new row), slot (the written
    buffer, valid through column c) and stop."""
    st = init_reference(Bn, k, Lm, START, FILL)
    bufs = [dict(run_seq=st["run_seq"], fin_seq=st["fin_seq"], slot=st["slot"]),
            dict(run_seq=torch.full_like(st["run_seq"], -1), fin_seq=torch.full_like(st["fin_seq"], -1), slot=torch.full_like(st["slot"], -1))]
    cur = {n: st[n] for n in ("run_score", "fin_score", "fin_flag", "fin_len", "unsat")}
    stop = st["stop"].clone()
    states = [dict({n: v.clone() for n, v in st.items()}, c=0)]
    rows = torch.arange(Bn * k)
    for c in range(1, Lm):
        inp, out = bufs[(c + 1) & 1], bufs[c & 1]
        if mut == "no swap at step 3" and c == 3:
            inp = out
        cs, ci = topk_reference(score_fn(c), cur["run_score"], k, V, 1, True)
        ref = update_reference(dict(cur, run_seq=inp["run_seq"], fin_seq=inp["fin_seq"]), cs, ci, c, cfg,
                               mut=mut if mut in ("pool tie to candidate", "fin_len kept") else None)
        par = (ref["par"] + torch.arange(Bn)[:, None] * k).reshape(-1)
        out["run_seq"], out["fin_seq"] = ref["run_seq"], ref["fin_seq"]
        out["slot"][:, :c] = inp["slot"][par, :c]
        if mut != "slot copied short":
            out["slot"][:, c] = rows.int()
        cur = {n: ref[n] for n in cur}
        stop[c] = ref["word"]
        states.append(dict(ref, c=c, cand_score=cs, cand_idx=ci, rows=par, slot=out["slot"].clone(), stop=stop.clone()))
        if not going(ref["word"], cfg["es"]):
            break
    return states


SEARCHES = ((1, 8, 6), (3, 16, 12), (4, 50, 70), (16, 40, 10))  # (k, V, Lm)
SEARCH_ES = (0, 1, 2)
SEARCH_LP = (0.0, 1.0, 2.0)


def scripted_scores(k, V, Lm, seed=0):
    """score_fn(c) -> [B*k, V] f32 on the 2^-4 grid in [-8, 0]: the EOS column is low (-16) except at chosen steps, where a third of
    the rows (which third moves with c) hold the best score of all, so beams finish at different lengths; one entry per row is -inf,
    as a processor leaves it.  Running scores stay sums of at most Lm grid values: exact in f32."""
    eos_steps = {2, 3, 5, Lm - 3, Lm - 2} if Lm < 20 else {8, 21, 40, Lm - 3}

    @functools.lru_cache(maxsize=None)
    def score_fn(c):
        g = torch.Generator().manual_seed(seed + 100 * c + k)
        x = _grid(g, 0, 128, B * k, V)
        x[:, EOS] = -16.0
        for r in range(B * k):
            if c in eos_steps and (r + c) % 3 == 0:
                x[r, EOS] = 0.0
            j = (7 * r + c) % V
            if j != EOS:
                x[r, j] = -float("inf")
        return x
    return score_fn


STATE_FIELDS = ("run_seq", "run_score", "tok", "par", "fin_score", "fin_flag", "unsat")


def state_mismatches(got, want, c, slot=True):
    """the names of the fields of a step's state (update_reference's keys, fin_len, slot, word) in which got differs from want,
    compared bit for bit; pool sequences and lengths count where the pool entry is flagged, the slot table through column c"""
    bad = [n for n in STATE_FIELDS if not torch.equal(got[n], want[n])]
    fl = want["fin_flag"]
    bad += [n for n in ("fin_seq", "fin_len") if not torch.equal(got[n][fl], want[n][fl])]
    if slot and not torch.equal(got["slot"][:, :c + 1], want["slot"][:, :c + 1]):
        bad.append("slot")
    if int(got["word"]) != int(want["word"]):
        bad.append("word")
    return bad


# ---- single-step scenarios ---------------------------------------------------------------------------------------------------------
UPDATE_KS = (1, 2, 3, 8, 16)
UPDATE_V = 50
# (pool full, heuristic unsatisfied, EOS candidate positions as functions of k): the table of tests/test_beam_gpu.py
SCENARIOS = ((False, True, lambda k: [0]), (False, True, lambda k: [k + 1]), (True, True, lambda k: [1, k]), (False, True, lambda k: []),
             (True, False, lambda k: [0]), (True, True, lambda k: [0, 1, 2, 3]))


def update_steps(Lm):
    return sorted({1, 2, Lm - 2, Lm - 1} | ({64, 65} if Lm == 70 else set()))


def random_state(Bn, k, Lm, g, c, full, unsat):
    run_seq = torch.randint(2, 50, (Bn, k, Lm), generator=g)
    run_seq[:, :, 0] = 0
    run_seq[:, :, c:] = 1
    fin_seq = torch.randint(2, 50, (Bn, k, Lm), generator=g)
    fin_seq[:, :, 0] = 0
    fin_flag = torch.rand(Bn, k, generator=g) < 0.5
    if full:
        fin_flag[:] = True
    fin_score = torch.where(fin_flag, -torch.rand(Bn, k, generator=g) * 4 - 0.5, torch.full((Bn, k), NEG))
    return dict(run_seq=run_seq, fin_seq=fin_seq, fin_flag=fin_flag, fin_score=fin_score,
                fin_len=torch.full((Bn, k), c - 1, dtype=torch.int32), unsat=torch.full((Bn, 1), bool(unsat)))


def random_candidates(Bn, k, V, g, eos_at):
    """2k candidates per sample, scores sorted and distinct, tokens distinct, EOS at the given positions"""
    K2 = 2 * k
    cs = -(torch.rand(Bn, K2, generator=g) * 0.3 + torch.arange(K2).float() * 0.5 + 0.2)
    beam = torch.randint(0, k, (Bn, K2), generator=g)
    tok = torch.stack([torch.randperm(V - 2, generator=g)[:K2] + 2 for _ in range(Bn)])
    tok[:, [p for p in eos_at if p < K2]] = EOS
    return cs, beam * V + tok


def tie_scenario(k, Lm, c, lp, g):
    """(state, cand_score, cand_idx) with exact ties, k >= 2: candidates 0 and 1 finish (EOS) with equal scores, pool entry 0 holds
    exactly their penalised score, candidates 2 and 3 run on with equal scores.  Grid values, so the f32 divide by c**lp of equal
    inputs gives equal outputs; the order is then beam_better's: pool entry, candidate 0, candidate 1; candidate 2 before 3."""
    K2 = 2 * k
    st = random_state(B, k, Lm, g, c, False, True)
    cs = torch.tensor([-1.0, -1.0, -2.0, -2.0] + [-2.5 - 0.5 * i for i in range(K2 - 4)])[None].repeat(B, 1)
    beam = torch.randint(0, k, (B, K2), generator=g)
    tok = torch.stack([torch.randperm(UPDATE_V - 2, generator=g)[:K2] + 2 for _ in range(B)])
    tok[:, :2] = EOS
    st["fin_flag"][:] = False
    st["fin_score"][:] = NEG
    st["fin_flag"][:, 0] = True
    st["fin_score"][:, 0] = _div(cs[:, 0], c ** lp)
    return st, cs, beam * UPDATE_V + tok
