"""Fixtures, fp64 reference and per-element bound for the K/V-cache decode attention (decode_attn_kernel<T, DK, SLOT> in
csrc/attn_t5.hip, entry klab_t5_beam_decode_attn): plain torch on the CPU, shared by tests/test_decode_attn_fixtures_cpu.py (which proves
what the GPU test takes for granted) and tests/test_decode_attn_exact_gpu.py.

Logical operands of one launch (fp64 tensors holding dtype-rounded values):
    q [R, H, dk]; K, V [S, rows, H, dk] (S slots or samples, rows >= Lk); bias [H, >= Lk] or None;
    kv_slot int32 [R, slot_ld] (key j of row r lies in slot kv_slot[r, j]) or None (then in sample r // kv_group).
reference(): softmax_j(q . k_j + bias_j) . v_j, unscaled (HF/t5:196-197), in fp64, in either addressing mode.

Exact fixture.  q[r, h] is 16 x a one-hot column, k is 0 or -16: a score is 0 on the chosen keys of (r, h) and -256 elsewhere.  With a
bias the keys of K's pattern are the chosen keys plus one key m_h per head that bias[h, m_h] = -256 takes out again (every other bias
entry is 0), so that the bias row of the wrong head changes the chosen set.  exp(-256) is 0 in f32, so the probabilities are exactly
1 / n on n in {1, 2, 4} chosen keys.  V[s, j, h, c] = sign(h, c) * 2^e(h, c) * m(s, j): the power of two and the sign are distinct per
(head, column) and |m| lies in one binade, so values of two (head, column) pairs never coincide; m encodes (slot, key) (f32: injective;
bf16: 31 values, distinct for any two slots of a key and for the pattern keys of a slot) and is positive on the keys some pattern
chooses, negative elsewhere.  The result is the mean of n values of one (head, column): an integer sum below 2^8 (bf16) or 2^15 (f32)
in units of the scale, exact in any order.  Which wrong reads the values tell apart is not argued here but tried:
tests/test_decode_attn_fixtures_cpu.py applies each mutation and demands a different number.

Random operands.  Row r's query is scaled so that the scores of row 0 stay within a few units (a flat softmax: every key and the
summation depth matter) and those of the last row reach about 60 (a peaked one: the exponential's error matters).  Three keys are
planted: Lk - 1, 64 (the first key of a second lap) and, in the logical operands only, row Lk (what a kernel that reads one key too many
finds; on the device that row is NaN).  A planted key scores half a unit below the row's largest other score for every (row, head) that
reads it, and its V is 8 x larger, so that dropping it, reading it from the wrong slot or weighting it wrongly moves the result by far
more than any rounding does.

Bound (per element, first order, nothing measured).  With u = 2^-24:
    eS_j = u ((dk + 2) sum_c |q_c k_jc| + 2 |s_j|)            dot product of dk terms, the bias addition
    eE_j = u (3 |s_j - max s| + 5 (laps + 1))                  every weight is a product of at most laps + 1 values of __expf whose
                                                               arguments add up to s_j - max s; per value the project's model
                                                               u (2 |x| + 4) (swin_exact_ref.SwinBounds) plus the argument's rounding
    D    = 2 laps + 6 + 4                                      in-lane multiply-adds, six shuffle levels, the scaling by f and by 1 / l
    f_j  = eS_j + eE_j + sum_i P_i (eS_i + eE_i) + 2 u D       relative error of the normalised weight of key j
    |ctx_c - ref_c| <= sum_j P_j f_j |v_jc|
A weight more than 87 below the maximum is below the smallest normal f32 and may be flushed to 0: + 2^-125 sum_j |v_jc|.
bf16 output: the f32 value y, |y - ref| <= tol (the f32 bound), is rounded once more.  Where ref lies farther than tol from a rounding
boundary the output is bf16(ref) itself; elsewhere it is off by at most tol and the rounding of y, an ulp (swin_exact_ref._flip):
bound = |bf16(ref) - ref| + tol + (ulp where ref is within tol of a boundary)."""
import functools
import math

import torch

from tests.swin_exact_ref import _flip

U24 = 2.0 ** -24
NEG = -256.0
R, H = 5, 3
LKS = (1, 6, 63, 64, 65, 130, 200)
DKS = (8, 16, 32, 64, 128)
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
# (form, kv_group): the self-attention layout with a slot table, the cross-attention layout with 1 and 2 rows per sample
FORMS = (("slot", 1), ("group", 1), ("group", 2))
MUTATIONS = ("drop_last", "read_extra", "slot_swap", "group_off", "bias_next_head", "no_rescale")


def shapes():
    """(Lk, dk): every Lk at dk 64 and 8, every dk at Lk 65 and 200"""
    out = [(Lk, dk) for dk in (64, 8) for Lk in LKS]
    out += [(Lk, dk) for dk in (16, 32, 128) for Lk in (65, 200)]
    return out


def cases(random_only=False):
    """(form, kv_group, Lk, dk, with_bias); random_only: the dk = 64 and dk = 128 rows"""
    return [(form, g, Lk, dk, wb) for (form, g) in FORMS for (Lk, dk) in shapes() for wb in (True, False)
            if not random_only or dk in (64, 128)]


def rows_of(kv_group):
    """the engine runs M = samples x kv_group rows: R = 5 rows where the group is 1, 6 (three samples) where it is 2"""
    return R if kv_group == 1 else 6


def slot_table(nrows, slot_ld):
    """int32 [nrows, slot_ld] over nrows slots, a bijection of the rows for every key: each (slot, key) is read by exactly one row.
    Entries at j >= Lk are slot numbers like any other (they point at rows the layout fills with NaN)."""
    r = torch.arange(nrows)[:, None]
    j = torch.arange(slot_ld)[None]
    return ((r + 3 * j + j // 64) % nrows).to(torch.int32)


def key_rows(nrows, Lk, kv_slot, kv_group):
    """int64 [nrows, Lk]: the slot or sample that key j of row r is read from"""
    if kv_slot is not None:
        return kv_slot[:, :Lk].long()
    return (torch.arange(nrows) // kv_group)[:, None].expand(nrows, Lk)


def reference(q, K, V, bias, Lk, kv_slot=None, kv_group=1):
    """fp64: ctx [R, H, dk], P [R, H, Lk], scores [R, H, Lk], |q|.|k| [R, H, Lk], the gathered V [R, Lk, H, dk]"""
    nrows = q.shape[0]
    s = key_rows(nrows, Lk, kv_slot, kv_group)
    j = torch.arange(Lk)[None].expand(nrows, Lk)
    Kr, Vr = K[s, j], V[s, j]  # [R, Lk, H, dk]
    sc = torch.einsum("rhc,rjhc->rhj", q, Kr)
    if bias is not None:
        sc = sc + bias[None, :, :Lk]
    P = torch.softmax(sc, -1)
    return dict(ctx=torch.einsum("rhj,rjhc->rhc", P, Vr), P=P, S=sc, absdot=torch.einsum("rhc,rjhc->rhj", q.abs(), Kr.abs()), V=Vr)


def lanes_reference(sc, Vr, rescale=True):
    """the kernel's own order in fp64: 64 lanes take keys lane, lane + 64, ... with an online softmax each, then merge.
    rescale=False leaves out the correction of what a lane has gathered when its maximum rises on a later lap (the mutation)."""
    nrows, nh, Lk = sc.shape
    dk = Vr.shape[-1]
    m = torch.full((nrows, nh, 64), -math.inf, dtype=torch.float64)
    l = torch.zeros(nrows, nh, 64, dtype=torch.float64)
    o = torch.zeros(nrows, nh, 64, dk, dtype=torch.float64)
    for lap in range((Lk + 63) // 64):
        n = min(64, Lk - lap * 64)
        s = sc[:, :, lap * 64:lap * 64 + n]
        v = Vr[:, lap * 64:lap * 64 + n].permute(0, 2, 1, 3)  # [R, H, n, dk]
        mn = torch.maximum(m[:, :, :n], s)
        corr = torch.exp(m[:, :, :n] - mn) if (rescale or lap == 0) else torch.ones_like(mn)
        pe = torch.exp(s - mn)
        l[:, :, :n] = l[:, :, :n] * corr + pe
        o[:, :, :n] = o[:, :, :n] * corr[..., None] + pe[..., None] * v
        m[:, :, :n] = mn
    mw = m.max(-1, keepdim=True).values
    f = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - mw))
    return (o * f[..., None]).sum(2) / (l * f).sum(-1, keepdim=True)


def mutated(mut, q, K, V, bias, Lk, kv_slot, kv_group, key=None):
    """the reference with one defect; K and V carry a row Lk.  key [R] (slot_swap): the key whose slot entry is replaced, per row"""
    nrows, nh = q.shape[0], q.shape[1]
    if mut == "drop_last":
        return reference(q, K, V, bias, Lk - 1, kv_slot, kv_group)["ctx"]
    if mut == "read_extra":
        return reference(q, K, V, bias, Lk + 1, kv_slot, kv_group)["ctx"]
    if mut == "slot_swap":
        t = (kv_slot if kv_slot is not None else key_rows(nrows, Lk, None, kv_group).to(torch.int32)).clone()
        rr = torch.arange(nrows)
        t[rr, key] = (t[rr, key] + 1) % K.shape[0]
        return reference(q, K, V, bias, Lk, t, 1)["ctx"]
    if mut == "group_off":  # (r + 1) / kv_group instead of r / kv_group
        s = ((torch.arange(nrows) + 1) // kv_group) % K.shape[0]
        t = s[:, None].expand(nrows, Lk + 1).to(torch.int32).contiguous()
        return reference(q, K, V, bias, Lk, t, 1)["ctx"]
    if mut == "bias_next_head":
        b = bias.clone()
        b[:nh - 1] = bias[1:]
        return reference(q, K, V, b, Lk, kv_slot, kv_group)["ctx"]
    if mut == "no_rescale":
        r = reference(q, K, V, bias, Lk, kv_slot, kv_group)
        return lanes_reference(r["S"], r["V"], rescale=False)
    raise KeyError(mut)


# ---- the exact fixture -------------------------------------------------------------------------------------------------------------
def patterns(Lk):
    """the chosen-key sets (1, 2 or 4 keys) of one Lk, at most 8.  In the order of the issue's list: key 0; key Lk - 1; both; keys 63 and
    64; one lane on two laps (5, 69); one lane on every lap (1, 65, 129, 193); lap 2 or 3 only, behind unchosen keys of the same
    lane (70; 135); lap 1 only with unchosen keys behind it (key 0 and key 3 whenever Lk > 67)."""
    if Lk == 1:
        return [(0,)]
    if Lk == 6:
        return [(0,), (5,), (0, 5), (2, 3)]
    if Lk in (63, 64):
        return [(0,), (Lk - 1,), (0, Lk - 1), (3,), (7, 8, 40, 41), (62,), (30, 31)]
    if Lk == 65:
        return [(0,), (64,), (0, 64), (63, 64), (3,), (7, 8, 63, 64), (62,), (1, 63)]
    if Lk == 130:
        return [(0,), (129,), (0, 129), (63, 64), (5, 69), (70,), (3,), (1, 65, 129, 128)]
    if Lk == 200:
        return [(0,), (199,), (63, 64), (5, 69), (1, 65, 129, 193), (70,), (135,), (3,)]
    raise KeyError(Lk)


def masked_keys(Lk, nh):
    """m_h: the key that bias row h takes out, from the keys no pattern uses, the highest lap first; adjacent heads differ"""
    used = {j for p in patterns(Lk) for j in p}
    free = sorted((j for j in range(Lk) if j not in used), key=lambda j: (-(j // 64), j))
    if len(free) < 2:
        return None  # Lk = 1: one key, probability 1 whatever the bias
    return [free[h % 2 * (len(free) // 2)] for h in range(nh)]


BF16_STEP = (1, 2)  # mantissa steps per pattern-key rank and per slot, modulo 31


def v_mantissa(dtype, S, Lk):
    """[S, Lk + 1] signed integers of one binade.  Keys that some pattern chooses are positive, all others (the masked keys and row
    Lk among them) negative: a key that joins a chosen set by mistake always moves the mean.  f32: 4096 + 256 slot + key.  bf16: 31
    values, 32 + (rank + 2 slot) mod 31 with rank counting the pattern keys (7 key for the others)."""
    used = sorted({j for p in patterns(Lk) for j in p})
    j = torch.arange(Lk + 1)
    s = torch.arange(S)[:, None]
    pos = torch.zeros(Lk + 1, dtype=torch.bool)
    pos[used] = True
    if dtype == torch.bfloat16:
        a = 7 * j
        a[used] = BF16_STEP[0] * torch.arange(len(used))
        m = 32 + (a[None] + BF16_STEP[1] * s) % 31
    else:
        m = 4096 + 256 * s + j[None]
    return torch.where(pos[None], m, -m)


class ExactFixture:
    pass


@functools.lru_cache(maxsize=None)
def exact_fixture(dtype_name, form, kv_group, Lk, dk, with_bias):
    """logical operands (rows Lk + 1: row Lk holds one more key that K's pattern chooses, for the read_extra mutation) and the written-down
    result.  chosen[r][h]: the tuple of keys with probability 1 / n."""
    dtype = DT[dtype_name]
    nrows = rows_of(kv_group)
    S = nrows if form == "slot" else nrows // kv_group
    pats = patterns(Lk)
    npat = len(pats)
    mk = masked_keys(Lk, H) if with_bias else None
    f = ExactFixture()
    f.Lk, f.dk, f.kv_group, f.form, f.rows = Lk, dk, kv_group, form, nrows
    f.kv_slot = slot_table(nrows, Lk + 3) if form == "slot" else None
    f.chosen = [[pats[(r * H + h) % npat] for h in range(H)] for r in range(nrows)]
    q = torch.zeros(nrows, H, dk, dtype=torch.float64)
    for r in range(nrows):
        for h in range(H):
            q[r, h, ((r * H + h) - h) % npat] = 16.0  # K's column c of head h holds pattern (c + h) % npat
    K = torch.full((S, Lk + 1, H, dk), -16.0, dtype=torch.float64)
    for h in range(H):
        for c in range(dk):
            keys = list(pats[(c + h) % npat]) + [Lk] + ([mk[h]] if mk else [])
            K[:, keys, h, c] = 0.0
    idx = (torch.arange(H)[:, None] * dk + torch.arange(dk)[None])[None, None]  # [1, 1, H, dk]
    scale = torch.where(idx % 2 == 0, 1.0, -1.0).double() * torch.pow(2.0, ((idx // 2) % 201 - 100).double())
    f.scale = scale[0, 0]
    V = v_mantissa(dtype, S, Lk)[:, :, None, None].double() * scale
    bias = None
    if with_bias:
        bias = torch.zeros(H, Lk + 1, dtype=torch.float64)
        for h in range(H if mk else 0):  # Lk = 1: one key, probability 1 whatever the bias; it stays 0
            bias[h, mk[h]] = NEG
    f.q, f.K, f.V, f.bias, f.masked = q, K, V, bias, mk
    srow = key_rows(nrows, Lk, f.kv_slot, kv_group)
    want = torch.zeros(nrows, H, dk, dtype=torch.float64)
    for r in range(nrows):
        for h in range(H):
            for j in f.chosen[r][h]:
                want[r, h] += V[srow[r, j], j, h]
            want[r, h] /= len(f.chosen[r][h])
    f.want = want
    return f


# ---- random operands ---------------------------------------------------------------------------------------------------------------
class RandomCase:
    pass


@functools.lru_cache(maxsize=None)
def random_case(dtype_name, form, kv_group, Lk, dk, with_bias, seed=0):
    dtype = DT[dtype_name]
    nrows = rows_of(kv_group)
    S = nrows if form == "slot" else nrows // kv_group
    g = torch.Generator().manual_seed(9100 + 131 * Lk + 7 * dk + 3 * kv_group + (form == "slot") + 2 * with_bias + seed)

    def rnd(x):
        return x.to(dtype).double()

    c = RandomCase()
    c.Lk, c.dk, c.kv_group, c.form, c.rows = Lk, dk, kv_group, form, nrows
    c.kv_slot = slot_table(nrows, Lk + 3) if form == "slot" else None
    top = 17.0 / math.sqrt(dk)
    rowscale = top * torch.linspace(0.1, 1.0, nrows, dtype=torch.float64)
    c.q = rnd(torch.randn(nrows, H, dk, generator=g, dtype=torch.float64) * rowscale[:, None, None])
    K = torch.randn(S, Lk + 1, H, dk, generator=g, dtype=torch.float64)
    V = torch.randn(S, Lk + 1, H, dk, generator=g, dtype=torch.float64)
    c.bias = (4.0 * torch.randn(H, Lk + 1, generator=g)).double() if with_bias else None
    c.planted = sorted({Lk - 1, Lk} | ({64} if Lk > 64 else set()))
    V[:, c.planted] *= 8.0
    # plant: every (row, head) that reads a planted key finds it half a unit below its largest other score
    table = c.kv_slot if form == "slot" else key_rows(nrows, Lk + 1, None, kv_group).to(torch.int32)
    r0 = reference(c.q, rnd(K), V, c.bias, Lk + 1, table, 1)
    S0 = r0["S"].clone()
    S0[:, :, c.planted] = -math.inf
    target = S0.max(-1).values - 0.5  # [R, H]
    if Lk == 1:
        target = torch.zeros(nrows, H, dtype=torch.float64)
    srow = table[:, :Lk + 1].long()
    for j in c.planted:
        for s in range(S):
            rows = (srow[:, j] == s).nonzero().flatten()
            for h in range(H):
                Q = c.q[rows, h]  # [g, dk]
                t = target[rows, h] - (c.bias[h, j] if with_bias else 0.0)
                K[s, j, h] = Q.T @ torch.linalg.solve(Q @ Q.T, t)
    c.K, c.V = rnd(K), rnd(V)
    return c


def bound(r, Lk, dk, dtype):
    """per-element bound [R, H, dk] from the fp64 reference r (see the header); bf16: against r["ctx"] for a kernel that rounds its f32 result"""
    P, S = r["P"], r["S"]
    laps = (Lk + 63) // 64
    eS = U24 * ((dk + 2) * r["absdot"] + 2.0 * S.abs())
    eE = U24 * (3.0 * (S - S.max(-1, keepdim=True).values).abs() + 5.0 * (laps + 1))
    D = 2 * laps + 6 + 4
    f = eS + eE + (P * (eS + eE)).sum(-1, keepdim=True) + 2.0 * U24 * D
    # + a weight below the smallest normal f32 (scores more than 87 under the maximum) may be flushed to 0
    tol = torch.einsum("rhj,rjhc->rhc", P * f, r["V"].abs()) + 2.0 ** -125 * r["V"].abs().sum(1)
    if dtype != torch.bfloat16:
        return tol
    x = r["ctx"]
    return (x.to(dtype).double() - x).abs() + _flip(x, dtype, tol)


def rejected(got, ref, bnd):
    """bool [R, H]: does some element of (row, head) leave the bound?"""
    return ((got - ref).abs() > bnd).any(-1)


# ---- device layouts (decode_rows in csrc/engine.cpp) ------------------------------------------------------------------------------------
NAN = float("nan")


def layout(c, dtype, device="cpu"):
    """the operands of fixture / case c as the decoding session lays them out; everything the kernel must not read is NaN.  Returns the
    tensors q, k, v (views of one buffer at the offsets the engine passes), the keyword arguments of ops.decode_attn except ctx and
    ctx_bstride, and the whole buffers (kv, q where it is not part of kv, bias) for whoever counts what is not NaN.
    slot form (self-attention at position t = Lk - 1 of a cache of Lt = Lk + 3 rows per slot): q | k | v interleaved, the new row's q
    in row t of the row's own slot, every other q block NaN, cache rows >= Lk NaN; bias row t of an [H, Lt, Lt] table, columns >= Lk NaN.
    group form (cross-attention of layer 1 of 3): k | v of the layer in its columns of [S, Le, 3 * 2 * inner], the other layers' NaN;
    q rows of pitch inner + 8 and bias rows of pitch Lk + 5 with NaN behind them."""
    Lk, dk, nrows = c.Lk, c.dk, c.rows
    inner = H * dk
    S = c.K.shape[0]
    kw = dict(R=nrows, H=H, Lk=Lk, dk=dk, kv_group=c.kv_group)
    if c.form == "slot":
        Lt, t = Lk + 3, Lk - 1
        cache = torch.full((S, Lt, 3 * inner), NAN, dtype=torch.float64)
        cache[:, :Lk, inner:2 * inner] = c.K[:, :Lk].reshape(S, Lk, inner)
        cache[:, :Lk, 2 * inner:] = c.V[:, :Lk].reshape(S, Lk, inner)
        cache[:, t, :inner] = c.q.reshape(nrows, inner)
        flat = cache.to(dtype).to(device).view(-1)
        q, k, v = flat[t * 3 * inner:], flat[inner:], flat[2 * inner:]
        kw.update(q_bstride=Lt * 3 * inner, kv_bstride=Lt * 3 * inner, ldk=3 * inner, kv_slot=c.kv_slot.to(device), slot_ld=Lt)
        assert c.kv_slot.shape == (nrows, Lt) and int(c.kv_slot.min()) >= 0 and int(c.kv_slot.max()) < S
        bias_row = None
        if c.bias is not None:
            tab = torch.full((H, Lt, Lt), NAN)
            tab[:, t, :Lk] = c.bias[:, :Lk].float()
            whole_bias = tab.to(device).view(-1)
            bias_row = whole_bias[t * Lt:]
            kw.update(bias_ld=Lt * Lt)
        whole = dict(kv=flat, q=None)
    else:
        nl, i = 3, 1
        kv_ld = nl * 2 * inner
        kv = torch.full((S, Lk, kv_ld), NAN, dtype=torch.float64)
        kv[:, :, i * 2 * inner:i * 2 * inner + inner] = c.K[:, :Lk].reshape(S, Lk, inner)
        kv[:, :, i * 2 * inner + inner:(i + 1) * 2 * inner] = c.V[:, :Lk].reshape(S, Lk, inner)
        flat = kv.to(dtype).to(device).view(-1)
        k, v = flat[i * 2 * inner:], flat[i * 2 * inner + inner:]
        qb = torch.full((nrows, inner + 8), NAN, dtype=torch.float64)
        qb[:, :inner] = c.q.reshape(nrows, inner)
        q = qb.to(dtype).to(device).view(-1)
        assert S * c.kv_group == nrows
        kw.update(q_bstride=inner + 8, kv_bstride=Lk * kv_ld, ldk=kv_ld)
        bias_row = None
        if c.bias is not None:
            bb = torch.full((H, Lk + 5), NAN)
            bb[:, :Lk] = c.bias[:, :Lk].float()
            whole_bias = bias_row = bb.to(device).view(-1)
            kw.update(bias_ld=Lk + 5)
        whole = dict(kv=flat, q=q)
    kw.update(bias_row=bias_row)
    whole.update(bias=whole_bias if c.bias is not None else None)
    return q, k, v, kw, whole


def read_like_the_kernel(q, k, v, kw):
    """the kernel's address arithmetic on the flat layout (CPU): q [R, H, dk], K and V [R, Lk, H, dk], bias [H, Lk] or None, as fp64"""
    nrows, nh, Lk, dk = kw["R"], kw["H"], kw["Lk"], kw["dk"]
    r = torch.arange(nrows)[:, None, None, None]
    j = torch.arange(Lk)[None, :, None, None]
    h = torch.arange(nh)[None, None, :, None]
    col = torch.arange(dk)[None, None, None, :]
    if kw.get("kv_slot") is not None:
        srow = kw["kv_slot"].view(-1)[(r * kw["slot_ld"] + j)].long()
    else:
        srow = r // kw["kv_group"]
    off = srow * kw["kv_bstride"] + j * kw["ldk"] + h * dk + col
    qo = (r * kw["q_bstride"] + h * dk + col)[:, 0]
    b = None
    if kw["bias_row"] is not None:
        b = kw["bias_row"][(h * kw["bias_ld"] + j)[0, :, :, 0].T].double()
    return q[qo].double(), k[off].double(), v[off].double(), b
