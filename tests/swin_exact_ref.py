"""Fixtures, fp64 references and per-element bounds for tests/test_swin_attn_exact_gpu.py (plain torch on the CPU;
tests/test_swin_exact_fixtures_cpu.py proves what the GPU tests take for granted about the fixtures).

The operation: Swin-V2 shifted-window cosine attention on a fused qkv [B R R, 3C] (HF/swinv2:389-455, 652-690) -- roll, window
partition, F.normalize(q) F.normalize(k)^T, * exp(min(logit_scale, ln 100)), + bias (dense [H, n, n] or gathered from the
(2w-1)^2 x H table), + the shift mask TWICE (-200), softmax, @ V, window reverse, un-roll; with R % w != 0 the grid is padded with
zero rows that still act as keys (k = 0, v = the value bias), the mask is built on the padded grid and the output is cropped.

Exact fixtures (everything is built in WINDOW space and scattered to token order through this file's own partition / roll, so the
fixtures share no index arithmetic with the kernels):
  "select"  scale = exp(0) = 1; q and k rows are signed one-hot vectors times a power of four (norms are powers of two, q-hat and
            k-hat are exact in bf16); the bias is -1000 except 0 on 1, 2 or 4 chosen keys per (head, query) whose cosine with the
            query is equal (0 for rows with several keys, +-1 for single-key rows of the dense form).  V and dctx are +-1 times a
            power of two that differs per image and window.  P is 1 / count on the chosen keys that the shift mask leaves, forward
            and every gradient are short sums of dyadic numbers, d logit_scale is exactly 0.
  "region"  bias 0 and every cosine 0: P = 1 / (keys in the query's shift region) -- 1/4, 1/8, 1/16 at w = 4 -- which pins the
            region arithmetic without any help from the bias.  Forward, and the f32 bias gradients (every pair of a region
            contributes to them; the other gradients are too long for a bf16 store).
  "onehot"  bias 0, logit_scale 5.0 (clamped: scale ~ 100); keys are the 2 hd signed one-hot codes, query i carries the code of
            key pi(i), every other score is ~100 lower: ctx = V[pi(i)] exactly.  Forward only (the scale is not exact).

Random operands: per-element bounds, the reference expression re-evaluated on absolute values times the unit roundoff of the
formats it passes through (SwinBounds; the derivation is in DESIGN.md section 1)."""
import functools
import math

import torch
import torch.nn.functional as F

from tests.exact_ref import U8, U24, bf16_exact, gen  # noqa: F401  (re-exported for the tests)

NEG = -1000.0
TINY = 2.0 ** -120      # below this a probability is flushed to zero in f32 while fp64 still holds it
LN100 = math.log(100.0)


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def geom(R, w):
    """(Rp, windows per side, windows per image) of the padded grid"""
    Rp = (R + w - 1) // w * w
    return Rp, Rp // w, (Rp // w) ** 2


def partition(x, w):
    """[B, Rp, Rp, F] -> [B nW, n, F] (HF/swinv2:146-155)"""
    B, Rp, _, Fd = x.shape
    return x.reshape(B, Rp // w, w, Rp // w, w, Fd).permute(0, 1, 3, 2, 4, 5).reshape(-1, w * w, Fd)


def reverse(xw, w, Rp):
    """[B nW, n, F] -> [B, Rp, Rp, F]"""
    Fd = xw.shape[-1]
    return xw.reshape(-1, Rp // w, Rp // w, w, w, Fd).permute(0, 1, 3, 2, 4, 5).reshape(-1, Rp, Rp, Fd)


def to_windows(tok, B, R, w, shift, fill=None):
    """token order [B R R, F] -> window space [B nW, n, F]: pad with zero rows (+ fill [F] on the padded positions), roll, partition"""
    Rp = geom(R, w)[0]
    x = F.pad(tok.reshape(B, R, R, -1), (0, 0, 0, Rp - R, 0, Rp - R))
    if fill is not None and Rp > R:
        pad = torch.ones(Rp, Rp, dtype=tok.dtype)
        pad[:R, :R] = 0
        x = x + pad[None, :, :, None] * fill
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    return partition(x, w)


def to_tokens(xw, B, R, w, shift):
    """window space -> token order: reverse, un-roll, crop"""
    Rp = geom(R, w)[0]
    x = reverse(xw, w, Rp)
    if shift > 0:
        x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
    return x[:, :R, :R].reshape(B * R * R, -1)


def real_positions(B, R, w, shift):
    """[B nW, n] bool: window slots that hold a real token (not a padded position)"""
    return to_windows(torch.ones(B * R * R, 1, dtype=torch.float64), B, R, w, shift)[..., 0] > 0


def region_ids(R, w, shift):
    """[nW, n] region of every window slot of the rolled, padded grid (HF/swinv2:620-643: slices 0:-w, -w:-shift, -shift:)"""
    Rp = geom(R, w)[0]
    img = torch.zeros(1, Rp, Rp, 1, dtype=torch.float64)
    if shift > 0:
        cnt = 0
        for hs in (slice(0, -w), slice(-w, -shift), slice(-shift, None)):
            for ws in (slice(0, -w), slice(-w, -shift), slice(-shift, None)):
                img[:, hs, ws, :] = cnt
                cnt += 1
    return partition(img, w)[..., 0].long()


def bands(w, shift):
    """[n] band pair of a window-local position: positions of one band pair share a region in EVERY window class"""
    j = torch.arange(w * w)
    if shift == 0:
        return torch.zeros(w * w, dtype=torch.long)
    return ((j // w) >= w - shift).long() * 2 + ((j % w) >= w - shift).long()


def rel_index(w):
    """[n, n] row of the bias table for (query i, key j) (HF/swinv2:480-490)"""
    j = torch.arange(w * w)
    y, x = j // w, j % w
    return (y[:, None] - y[None, :] + w - 1) * (2 * w - 1) + (x[:, None] - x[None, :] + w - 1)


def table_to_dense(table, w):
    n, H = w * w, table.shape[1]
    return table[rel_index(w).reshape(-1)].reshape(n, n, H).permute(2, 0, 1)


def dense_to_table(dbias, w):
    """sum a dense [H, n, n] gradient into the table's rows: [(2w-1)^2, H]"""
    H = dbias.shape[0]
    out = torch.zeros((2 * w - 1) ** 2, H, dtype=dbias.dtype)
    return out.index_add_(0, rel_index(w).reshape(-1), dbias.permute(1, 2, 0).reshape(-1, H))


def heads(xw, H):
    """[BW, n, C] -> [BW, H, n, hd]"""
    BW, n, C = xw.shape
    return xw.reshape(BW, n, H, C // H).transpose(1, 2)


def unheads(x):
    BW, H, n, hd = x.shape
    return x.transpose(1, 2).reshape(BW, n, H * hd)


# ---- the fp64 reference --------------------------------------------------------------------------------------------------------
def _round_st(x, dt):
    """round to the operand dtype, straight-through gradient"""
    if dt is None:
        return x
    return x + (x.detach().to(dt).double() - x.detach())


def swin_reference(qkv, logit_scale, B, R, w, shift, H, C, bias=None, table=None, v_bias=None, round_dtype=None):
    """Plain fp64 shifted-window cosine attention.  qkv [B R R, 3C], logit_scale [H], bias [H, n, n] or table [(2w-1)^2, H],
    v_bias [C] (the value of a padded key).  round_dtype: q-hat and k-hat are rounded to it before the score product, as the
    kernels do (attn_swin.hip:95).  Returns ctx [B R R, C], lse [B nW H n] and the window-space companions the bounds need."""
    n = w * w
    Rp, _nWr, nW = geom(R, w)
    fill = None
    if Rp > R and v_bias is not None:
        fill = torch.cat([torch.zeros(2 * C, dtype=torch.float64), v_bias])
    xw = to_windows(qkv, B, R, w, shift, fill)
    q, k, v = (heads(xw[..., i * C:(i + 1) * C], H) for i in range(3))
    qh0, kh0 = F.normalize(q, dim=-1, eps=1e-12), F.normalize(k, dim=-1, eps=1e-12)
    qh, kh = _round_st(qh0, round_dtype), _round_st(kh0, round_dtype)
    scale = torch.clamp(logit_scale, max=LN100).exp().view(1, H, 1, 1)
    cos = qh @ kh.transpose(-1, -2)
    bd = bias if bias is not None else table_to_dense(table, w)
    reg = region_ids(R, w, shift)
    other = (reg[:, :, None] != reg[:, None, :])                      # [nW, n, n]
    other = other[None].expand(B, nW, n, n).reshape(B * nW, 1, n, n)
    S = cos * scale + bd[None] + other.double() * -100.0 + other.double() * -100.0   # the mask is added on two consecutive lines
    lse = torch.logsumexp(S, -1)
    P = (S - lse[..., None]).exp()
    ctxw = P @ v
    ctx = to_tokens(unheads(ctxw), B, R, w, shift)
    return dict(ctx=ctx, lse=lse, P=P, S=S, cos=cos, qh=qh, kh=kh, qh0=qh0, kh0=kh0, qn=q.norm(dim=-1), kn=k.norm(dim=-1), v=v,
                scale=scale, other=other, bias_dense=bd, real=real_positions(B, R, w, shift))


def swin_reference_grads(qkv, logit_scale, dctx, B, R, w, shift, H, C, bias=None, table=None, v_bias=None, round_dtype=None):
    """the reference and, through autograd in fp64, d qkv, d bias or d table, d logit_scale, d v_bias"""
    leaves = dict(qkv=qkv.clone().requires_grad_(True), ls=logit_scale.clone().requires_grad_(True))
    if bias is not None:
        leaves["bias"] = bias.clone().requires_grad_(True)
    if table is not None:
        leaves["table"] = table.clone().requires_grad_(True)
    if v_bias is not None:
        leaves["v_bias"] = v_bias.clone().requires_grad_(True)
    r = swin_reference(leaves["qkv"], leaves["ls"], B, R, w, shift, H, C, leaves.get("bias"), leaves.get("table"), leaves.get("v_bias"),
                       round_dtype)
    r["ctx"].backward(dctx)
    g = {"d" + k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in r.items()}
    out.update(g)
    out["dow"] = heads(to_windows(dctx, B, R, w, shift), H)
    return out


def fused_qkv(x, wqkv, bqkv):
    """q | k | v of the fused projection kernels in fp64, WITHOUT a bf16 rounding before the normalisation (the documented difference
    between klab_swin_qkv_attn_fused and the two-kernel path)"""
    y = x @ wqkv.T
    return y if bqkv is None else y + bqkv[None]


# ---- per-element bounds --------------------------------------------------------------------------------------------------------
def _flip(x0, dt, tol):
    """The kernel normalises in f32 and THEN rounds q-hat / k-hat to the operand dtype: where the fp64 value lies within the f32
    error `tol` (absolute, per element) of a rounding boundary the kernel may round the other way, which is a whole ulp.  Returns
    the per-element slack: the ulp where a flip is possible, tol elsewhere."""
    if dt != torch.bfloat16:
        return tol
    r = x0.to(dt).double()
    ulp = 2.0 ** (torch.floor(torch.log2(x0.abs().clamp_min(1e-300))) - 7)
    near = (0.5 * ulp - (x0 - r).abs()) <= tol
    return torch.where(near, ulp, torch.zeros_like(ulp)) + tol


class SwinBounds:
    """Bounds for one call, all from the fp64 reference r (swin_reference_grads).  dtype: the operand / output dtype of the kernel;
    mfma: the matrix-core kernels, which feed bf16(P) and bf16(dS) to the second products and keep dQ-hat / dK-hat / dV in bf16
    scratch; fused: q | k | v come from the in-kernel projection (eq, ek: its f32 error relative to |q|, |k| per row, and V is
    rounded to bf16 once more).  Every term is first-order; `margin` (per output, set from the measured worst ratios recorded in
    DESIGN.md section 1) multiplies the whole."""

    def __init__(self, r, B, R, w, shift, H, C, dtype, mfma=False, eq=None, ek=None, v_rounded=False):
        self.r, self.g = r, (B, R, w, shift, H, C)
        n, hd = w * w, C // H
        bf = dtype == torch.bfloat16
        self.bf, self.mfma, self.n, self.hd = bf, mfma, n, hd
        P, S, cos, s = r["P"], r["S"], r["cos"], r["scale"]
        qa, ka = r["qh"].abs(), r["kh"].abs()
        # q-hat / k-hat as the kernel holds them: f32 normalisation ((hd + 8) roundings), then the operand rounding
        tq = U24 * (hd + 8) * r["qh0"].abs() + (0.0 if eq is None else eq[..., None] * 1.0)
        tk = U24 * (hd + 8) * r["kh0"].abs() + (0.0 if ek is None else ek[..., None] * 1.0)
        self.fq, self.fk = _flip(r["qh0"], dtype, tq), _flip(r["kh0"], dtype, tk)
        absdot = qa @ ka.transpose(-1, -2)
        # absolute error of a score: the f32 dot product and scale, the f32 additions of bias and mask, the operand flips
        eS = U24 * (hd + 8) * s * absdot + U24 * (S.abs() + r["bias_dense"].abs()[None] + 200.0 * r["other"].double() + 4.0) \
            + s * (self.fq @ ka.transpose(-1, -2) + qa @ self.fk.transpose(-1, -2))
        # __expf(x) = exp2(x log2 e): the product's rounding and the constant's, 2 * 2^-24 |x|, plus the instruction's ulp
        eE = U24 * (2.0 * (S - r["lse"][..., None]).abs() + 4.0)
        rowavg = (P * (eS + eE)).sum(-1, keepdim=True)
        self.e_lse = rowavg[..., 0] + U24 * (n + 2.0 * r["lse"].abs() + 16.0)
        f = eS + eE + self.e_lse[..., None]
        self.EP = f * P + TINY                        # |P_kernel - P|, P as the kernel's f32 registers hold it
        self.P8 = U8 * P if (bf and mfma) else 0.0    # + the bf16 rounding of P in front of the second product
        va = r["v"].abs()
        self.ev = U8 * va if v_rounded else torch.zeros_like(va)
        self.ctxw = (self.EP + self.P8) @ va + P @ self.ev + U24 * (n + 2) * (P @ va)
        if bf:
            self.ctxw = self.ctxw + U8 * (P @ r["v"]).abs()
        if "dow" not in r:
            return
        do = r["dow"]
        doa = do.abs()
        ctxw_ref = P @ r["v"]
        dP = do @ r["v"].transpose(-1, -2)
        delta = (do * ctxw_ref).sum(-1, keepdim=True)
        e_dP = U24 * (hd + 2) * (doa @ va.transpose(-1, -2))
        # delta = dO . ctx from the STORED context (tiled, streaming and matrix-core kernels), or sum_j P_ij dP_ij (one-tile kernel):
        # either way within dO's share of the context bound
        e_delta = (doa * self.ctxw).sum(-1, keepdim=True) + U24 * (hd + 2) * (do * ctxw_ref).abs().sum(-1, keepdim=True)
        dS = P * (dP - delta)
        self.dS = dS
        self.e_dS = self.EP * (dP - delta).abs() + P * (e_dP + e_delta) + 2.0 * U24 * dS.abs()
        if bf and mfma:
            self.e_dS = self.e_dS + U8 * dS.abs()     # dS is rounded to bf16 for the dQ / dK products and the stored-dS slab
        real = r["real"][:, None, :, None].double()   # padded queries carry no gradient
        self.e_dS = self.e_dS * real
        dSr = dS * real
        st = 2.0 if (bf and mfma) else 1.0            # bf16 scratch of dQ-hat / dK-hat / dV on top of the output store
        dqh = s * (dSr @ r["kh"])
        e_dqh = s * (self.e_dS @ ka) + U24 * (n + 4) * s * (dSr.abs() @ ka) + (U8 * dqh.abs() if (bf and mfma) else 0.0)
        dkh = s * (dSr.transpose(-1, -2) @ r["qh"])
        e_dkh = s * (self.e_dS.transpose(-1, -2) @ qa) + U24 * (n + 4) * s * (dSr.abs().transpose(-1, -2) @ qa) \
            + (U8 * dkh.abs() if (bf and mfma) else 0.0)
        self.dq = self._jac(r["qh"], r["qh0"], dqh, e_dqh, r["qn"], self.fq)
        self.dk = self._jac(r["kh"], r["kh0"], dkh, e_dkh, r["kn"], self.fk)
        dv = P.transpose(-1, -2) @ (do * real)
        self.dv = (self.EP + self.P8).transpose(-1, -2) @ (doa * real) + U24 * (n + 2) * (P.transpose(-1, -2) @ (doa * real)) \
            + (st * U8 * dv.abs() if bf else 0.0)
        self.dvw = dv
        # d logit_scale = scale sum dS cos (one-tile / tiled kernels) or scale sum_i dQ-hat_i . q-hat_i (matrix-core path)
        term = self.e_dS * cos.abs() + dSr.abs() * U24 * (hd + 2) * absdot
        flips = (self.fq * (dSr.abs() @ ka)).sum((0, 2, 3)) + (self.fk * (dSr.abs().transpose(-1, -2) @ qa)).sum((0, 2, 3))
        e_ls = s[0, :, 0, 0] * (term.sum((0, 2, 3)) + flips)
        if bf and mfma:
            e_ls = e_ls + U8 * ((dqh.abs() * qa).sum((0, 2, 3)))
        cnt = dS.shape[0] * n
        self.dls = e_ls + U24 * (math.log2(cnt) + 8) * s[0, :, 0, 0] * (dSr * cos).abs().sum((0, 2, 3))
        self.dbias = self.e_dS.sum(0) + U24 * (math.log2(dS.shape[0]) + 2) * dSr.abs().sum(0)

    def _jac(self, xh, xh0, dxh, e_dxh, xn, fx):
        """x-hat = x / |x|: dx = (dx-hat - x-hat (x-hat . dx-hat)) / |x|.  The reference differentiates through the unrounded x-hat
        (straight-through rounding), the kernels use the rounded one on both sides: fx, the rounding slack of x-hat, enters twice."""
        xa = xh.abs()
        inv = torch.where(xn > 0, 1.0 / xn.clamp_min(1e-300), torch.zeros_like(xn))[..., None]
        dot = (xa * dxh.abs()).sum(-1, keepdim=True)
        rnd = (U8 * xa if self.bf else 0.0) + fx
        e = e_dxh + xa * (xa * e_dxh).sum(-1, keepdim=True) + rnd * dot + xa * (rnd * dxh.abs()).sum(-1, keepdim=True) \
            + U24 * (self.hd + 6) * (dxh.abs() + xa * dot)
        out = e * inv
        if self.bf:
            full = (dxh - xh0 * (xh0 * dxh).sum(-1, keepdim=True)) * inv
            out = out + U8 * full.abs()
        return out

    # token-order / parameter-shaped forms
    def tok(self, xw):
        B, R, w, shift, _H, _C = self.g
        return to_tokens(unheads(xw), B, R, w, shift)

    def ctx(self):
        return self.tok(self.ctxw)

    def dqkv(self):
        return torch.cat([self.tok(self.dq), self.tok(self.dk), self.tok(self.dv)], dim=1)

    def dtable(self):
        return dense_to_table(self.dbias, self.g[2]) + U24 * 8 * dense_to_table(self.dS.abs().sum(0), self.g[2])

    def dv_bias(self):
        """sum of d v over the padded keys (f32 atomics of f32 or bf16 values)"""
        pad = (~self.r["real"])[:, None, :, None].double()
        e = (self.dv * pad).sum((0, 2)) + U24 * 16 * (self.dvw.abs() * pad).sum((0, 2))
        return e.reshape(-1)


# ---- exact fixtures ------------------------------------------------------------------------------------------------------------
def _codes(axis, sign, mag, hd):
    """signed one-hot rows: sign * mag at column axis"""
    out = torch.zeros(*axis.shape, hd, dtype=torch.float64)
    out.scatter_(-1, axis[..., None], (sign * mag)[..., None])
    return out


def table_offsets(h, w):
    """the (a, b) of head h's chosen offset set {0, a} x {0, b} in the table form: small and large, both signs"""
    opts = [(1, 1), (-1, 2), (w - 1, -1), (-(w // 2), w // 2), (2, -(w - 1)), (0, 1), (1, 0)]
    return opts[h % len(opts)]


class SwinFixture:
    """One exact fixture at one shape (see the module docstring).  Token-order inputs qkv [B R R, 3C], dctx [B R R, C], bias [H, n, n]
    or table, logit_scale [H], v_bias [C] (padded grids) -- all fp64 and bf16-exact; the expectations ctx, lse, and for "select"
    dqkv, dbias / dtable, dv_bias are written down from P = 1 / count, never computed through exp."""

    def __init__(self, kind, B, R, w, shift, H, C, form="dense", shared=False, perm=1, seed=0):
        assert kind in ("select", "region", "onehot") and form in ("dense", "table")
        self.kind, self.form, self.geo = kind, form, (B, R, w, shift, H, C)
        n, hd = w * w, C // H
        Rp, _nWr, nW = geom(R, w)
        BW = B * nW
        g = gen(7000 + seed)
        padded = Rp > R
        bd = bands(w, shift)
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)
        pm = lambda *s: (2 * ri(0, 1, *s) - 1).double()
        S0 = (1 if shared else BW, H, n)
        # ---- q, k codes
        if kind == "onehot":
            assert n <= 2 * hd and not padded and form == "dense"
            code = torch.stack([torch.stack([torch.randperm(2 * hd, generator=g)[:n] for _ in range(H)]) for _ in range(S0[0])])
            kax, ksg = code // 2, (1 - 2 * (code % 2)).double()
            pi = torch.arange(n)
            for b_ in range(4):   # a cyclic shift inside every band pair: the chosen key is never masked in any window class
                idx = (bd == b_).nonzero()[:, 0]
                if len(idx):
                    pi[idx] = idx.roll(-perm)
            self.pi = pi
            qax, qsg = kax[..., pi], ksg[..., pi]
        else:
            kax, ksg = ri(hd // 2, hd - 1, *S0), pm(*S0)      # keys in the upper half of the head, queries in the lower: cosine 0
            qax, qsg = ri(0, hd // 2 - 1, *S0), pm(*S0)
        kmag, qmag = 4.0 ** ri(-1, 1, *S0).double(), 4.0 ** ri(-1, 2, *S0).double()
        # ---- chosen keys -> bias
        self.ls = torch.zeros(H, dtype=torch.float64)
        chosen = torch.ones(H, n, n, dtype=torch.bool)
        if kind == "onehot":
            self.ls[:] = 5.0
        if kind == "select":
            chosen = torch.zeros(H, n, n, dtype=torch.bool)
            single_head = H - 1 if H >= 2 else -1     # this head gets logit_scale 5.0 (clamped) and single-key rows only
            if single_head >= 0:
                self.ls[single_head] = 5.0
            if form == "table":
                j = torch.arange(n)
                y, x = j // w, j % w
                for h in range(H):
                    a, b_ = (0, 0) if h == single_head else table_offsets(h, w)
                    for da in {0, a}:
                        for db in {0, b_}:
                            chosen[h] |= ((y[None, :] - y[:, None]) == da) & ((x[None, :] - x[:, None]) == db)
            else:
                for h in range(H):
                    for i in range(n):
                        same = (bd == bd[i]).nonzero()[:, 0]
                        diff = (bd != bd[i]).nonzero()[:, 0]
                        pick = lambda pool, m: pool[torch.randperm(len(pool), generator=g)[:m]]
                        typ = 0 if h == single_head else (i + h) % 4
                        if i == 0 or i == n - 1:
                            keys = torch.tensor([i])      # the first and the last key of the window are chosen by some row
                        elif i == 1:
                            keys = same[-1:]              # ... and the last key of the first band
                        elif typ == 0 or len(same) < 2:
                            keys = pick(same, 1)
                        elif typ == 2 and len(diff):
                            keys = torch.cat([pick(same, 1), pick(diff, 1)])
                        elif typ == 3 and len(same) >= 4:
                            keys = pick(same, 4)
                        else:
                            keys = pick(same, 2)
                        chosen[h, i, keys] = True
        self.chosen = chosen
        bias = torch.where(chosen, 0.0, NEG).double() if kind == "select" else torch.zeros(H, n, n, dtype=torch.float64)
        if form == "table":
            tab = torch.full(((2 * w - 1) ** 2, H), NEG if kind == "select" else 0.0, dtype=torch.float64)
            if kind == "select":
                idx = rel_index(w)
                for h in range(H):
                    tab[idx[chosen[h]], h] = 0.0
                assert torch.equal(table_to_dense(tab, w) == 0, chosen)
            self.table, self.bias = tab, None
        else:
            self.table, self.bias = None, bias
        if kind == "select" and form == "dense":
            # single-key rows: the query carries +- the code of its key (cosine +-1, lse = +-1 where the scale is 1)
            cnt = chosen.sum(-1)
            for h in range(H):
                for i in (cnt[h] == 1).nonzero()[:, 0].tolist():
                    j = int(chosen[h, i].nonzero()[0, 0])
                    qax[:, h, i] = kax[:, h, j]
        q = _codes(qax, qsg, qmag, hd).expand(BW, H, n, hd)
        k = _codes(kax, ksg, kmag, hd).expand(BW, H, n, hd)
        # ---- V, dctx: +-1 times a power of two per image and window
        e_v = (2.0 ** (torch.arange(BW) % 4).double()).view(BW, 1, 1, 1)
        e_d = (2.0 ** ((torch.arange(BW) // 2) % 3).double()).view(BW, 1, 1, 1)
        v0, d0 = pm(S0[0], H, n, hd), pm(S0[0], H, n, hd)
        self.v_unit, self.e_v = v0, e_v     # the fused fixtures rebuild V from these
        v, do = v0.expand(BW, H, n, hd) * e_v, d0.expand(BW, H, n, hd) * e_d
        self.v_bias = pm(C) * 2.0 if padded else None
        self.q_w, self.k_w, self.v_w = q, k, v
        self.qkv = to_tokens(torch.cat([unheads(q), unheads(k), unheads(v)], -1), B, R, w, shift).contiguous()
        self.dctx = to_tokens(unheads(do), B, R, w, shift).contiguous()
        self._expect()

    def _expect(self):
        B, R, w, shift, H, C = self.geo
        n = w * w
        _Rp, _nWr, nW = geom(R, w)
        fill = None if self.v_bias is None else torch.cat([torch.zeros(2 * C, dtype=torch.float64), self.v_bias])
        xw = to_windows(self.qkv, B, R, w, shift, fill)
        q, k, v = (heads(xw[..., i * C:(i + 1) * C], H) for i in range(3))
        qn, kn = q.norm(dim=-1, keepdim=True), k.norm(dim=-1, keepdim=True)
        qh, kh = q / qn.clamp_min(1e-12), k / kn.clamp_min(1e-12)
        self.qh, self.kh = qh, kh
        reg = region_ids(R, w, shift)
        same = (reg[:, :, None] == reg[:, None, :])[None].expand(B, nW, n, n).reshape(B * nW, 1, n, n)
        cos = qh @ kh.transpose(-1, -2)
        self.cos = cos
        if self.kind == "onehot":
            alive = (cos == 1.0) & same
        else:
            alive = self.chosen[None] & same
        cnt = alive.sum(-1, keepdim=True).double()
        self.cnt = cnt[..., 0]
        P = alive.double() / cnt
        self.P = P
        scale = torch.clamp(self.ls, max=LN100).exp().view(1, H, 1, 1)
        score = torch.where(alive, cos * scale, -math.inf).amax(-1)    # the score the surviving keys of a row share
        self.alive_scores_equal = bool((torch.where(alive, cos * scale, score[..., None]) == score[..., None]).all())
        self.lse = score + cnt[..., 0].log()
        self.single = (cnt[..., 0] == 1)
        ctxw = P @ v
        self.ctx_w = ctxw
        self.ctx = to_tokens(unheads(ctxw), B, R, w, shift)
        self.real = real_positions(B, R, w, shift)
        if self.kind == "onehot":
            return
        # "region": only the f32 bias gradients are exact (dS is a multiple of 1 / 256 or finer: too long for a bf16 store)
        real = self.real[:, None, :, None].double()
        do = heads(to_windows(self.dctx, B, R, w, shift), H)
        dP = do @ v.transpose(-1, -2)
        delta = (do * ctxw).sum(-1, keepdim=True)
        dS = P * (dP - delta) * real
        self.dS = dS
        dqh, dkh = scale * (dS @ kh), scale * (dS.transpose(-1, -2) @ qh)
        inv = lambda nrm: torch.where(nrm > 0, 1.0 / nrm.clamp_min(1e-300), torch.zeros_like(nrm))
        dq = (dqh - qh * (qh * dqh).sum(-1, keepdim=True)) * inv(qn)
        dk = (dkh - kh * (kh * dkh).sum(-1, keepdim=True)) * inv(kn)
        dv = P.transpose(-1, -2) @ (do * real)
        self.dqh, self.dkh = dqh, dkh
        self.dqkv = torch.cat([to_tokens(unheads(x), B, R, w, shift) for x in (dq, dk, dv)], 1)
        self.dbias = dS.sum(0)
        self.dtable = dense_to_table(self.dbias, w)
        self.dls = (dS * cos).sum((0, 2, 3)) * scale.view(-1) * (self.ls <= LN100)
        pad = (~self.real)[:, None, :, None].double()
        self.dv_bias = (dv * pad).sum((0, 2)).reshape(-1)

    def reference(self, grads=True):
        B, R, w, shift, H, C = self.geo
        if grads:
            return swin_reference_grads(self.qkv, self.ls, self.dctx, B, R, w, shift, H, C, self.bias, self.table, self.v_bias)
        return swin_reference(self.qkv, self.ls, B, R, w, shift, H, C, self.bias, self.table, self.v_bias)

    def fused_operands(self):
        """x [B R R, C] and wqkv [3C, C] that make the projection kernels compute this fixture's q | k | v: x is a per-window
        power of two times the one-hot code of the token's window position, column j of wqkv holds position j's q | k | v.  Needs a
        fixture built with shared=True (one pattern for all windows), n <= C and no padding."""
        B, R, w, shift, H, C = self.geo
        n = w * w
        assert n <= C and self.q_w.shape[0] == B * geom(R, w)[2]
        BW = self.q_w.shape[0]
        xw = torch.zeros(BW, n, C, dtype=torch.float64)
        xw[:, torch.arange(n), torch.arange(n)] = 1.0
        xw = xw * self.e_v.view(BW, 1, 1)
        wq = torch.zeros(3 * C, C, dtype=torch.float64)
        for i, src in enumerate((self.q_w, self.k_w, self.v_w / self.e_v)):
            wq[i * C:(i + 1) * C, :n] = unheads(src[:1])[0].T
        return to_tokens(xw, B, R, w, shift).contiguous(), wq


@functools.lru_cache(maxsize=None)
def swin_fixture(kind, B, R, w, shift, H, C, form="dense", shared=False, perm=1, seed=0):
    """Cached: callers must not write into what they get.  "select" fixtures are redrawn (next seed) until every expected output
    is a bf16 number -- sums of a few dS values on one k-hat component can exceed 8 significant bits."""
    for s in range(seed, seed + 50):
        f = SwinFixture(kind, B, R, w, shift, H, C, form, shared, perm, s)
        if kind != "select" or all(bf16_exact(x) for x in (f.ctx, f.dqkv, f.dS, f.dqh, f.dkh)):
            return f
    raise AssertionError("no bf16-exact fixture in 50 draws")


@functools.lru_cache(maxsize=None)
def swin_randn(B, R, w, shift, H, C, form, seed=0):
    """randn qkv / dctx rounded to bf16, bias 16 sigmoid(randn) (dense or table), logit_scale around ln 10 with head 0 at 5.0
    (above ln 100: clamped, scale 100, zero gradient), a value bias for padded grids"""
    g = gen(8000 + seed)
    n = w * w
    rb = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).double()
    qkv, dctx = rb(B * R * R, 3 * C), rb(B * R * R, C)
    ls = (math.log(10.0) + 0.3 * torch.randn(H, generator=g)).float().double()
    if H >= 2:
        ls[0] = 5.0
    bias = table = None
    if form == "table":
        table = (16 * torch.sigmoid(torch.randn((2 * w - 1) ** 2, H, generator=g))).float().double()
    else:
        bias = (16 * torch.sigmoid(torch.randn(H, n, n, generator=g))).float().double()
    v_bias = (0.5 * torch.randn(C, generator=g)).to(torch.bfloat16).double() if R % w else None
    return dict(qkv=qkv, dctx=dctx, ls=ls, bias=bias, table=table, v_bias=v_bias)


@functools.lru_cache(maxsize=None)
def swin_randn_reference(B, R, w, shift, H, C, form, dtype_name, seed=0):
    d = swin_randn(B, R, w, shift, H, C, form, seed)
    dt = torch.bfloat16 if dtype_name == "bf16" else torch.float32
    return swin_reference_grads(d["qkv"], d["ls"], d["dctx"], B, R, w, shift, H, C, d["bias"], d["table"], d["v_bias"], round_dtype=dt)


# ---- the shapes: the smallest that reach each dispatcher rule (klab_swin_attn_fwd / _bwd, swin_use_large, swin_flash_ok,
# swin_bwd_mfma_ok, launch_tiled).  B = 2 throughout so that a batch-stride error shows. -------------------------------------------
B_ = 2
# (R, w, shift): one window of 4 tokens; w = 2 shifted; w = 4 (R = 2w: all four window classes) plain and shifted; R = 3w (an
# interior window between two edge windows); w = 7 (49 tokens, padded to 64 keys in the matrix-core kernels); w = 8 (exactly one tile)
SMALL_GEO = [(2, 2, 0), (4, 2, 1), (8, 4, 0), (8, 4, 2), (12, 4, 2), (14, 7, 0), (14, 7, 3), (16, 8, 0), (16, 8, 4)]
# (dtype, head dim) -> forward kernel: swin_attn_fwd_kernel<float, 16 / 32>, swin_attn_fwd_kernel<bf16, 16> (vector ALU),
# swin_attn_fwd_mfma32 (bf16, 32; swin_attn_fwd_kernel<bf16, 32> is unreachable: hd == 32 and n <= 64 always takes the MFMA
# form, n > 64 the tiled kernels).  Backward: swin_attn_bwd_kernel<T, HD> with mfma=False, and for (bf16, 32) with mfma=True the
# gather -> t5_attn_bwd_mfma<32> -> klab_dbias_reduce -> scatter sequence (+ swin_bias_mask_kernel when shift > 0)
SMALL_CFG = [("f32", 16), ("f32", 32), ("bf16", 16), ("bf16", 32)]
# windows of more than 64 tokens (swin_use_large: w w > 64), padded grids (R % w != 0) and the table form: the tiled kernels
# swin_attn_fwd_tiled / _bwd_dq_tiled / _bwd_dkv_tiled<T, HD>; (bf16, 32, table, mfma=True) the streaming matrix-core kernels.
# n = 81: one full 64-key block + a ragged one; n = 144: three blocks, the last ragged; R = 9 / w = 4 and R = 10 / w = 6: padded
LARGE_GEO = [(9, 9, 0), (18, 9, 4), (12, 12, 0), (24, 12, 6), (9, 4, 2), (10, 6, 3), (10, 6, 0)]
# the fused projection kernels klab_swin_qkv_attn_fused / _img<C>: C = 64, 128 (weights in registers), 256 (k block by k block)
FUSED_GEO = [(14, 7, 0), (14, 7, 3), (16, 8, 0), (16, 8, 4)]
FUSED_C = [64, 128, 256]


def heads_for(R, w, hd):
    """H: 8 for the one-window w = 2 case (n = 4, H = 8), else 2"""
    return 8 if (R, w) == (2, 2) else 2


def small_cases():
    return [(dn, R, w, s, heads_for(R, w, hd), heads_for(R, w, hd) * hd) for (R, w, s) in SMALL_GEO for (dn, hd) in SMALL_CFG]


def large_cases():
    """(dtype, R, w, shift, H, C, form, mfma)"""
    out = []
    for (R, w, s) in LARGE_GEO:
        for dn, hd in SMALL_CFG:
            for form in ("table", "dense"):
                out.append((dn, R, w, s, 2, 2 * hd, form, False))
        out.append(("bf16", R, w, s, 2, 64, "table", True))
    # a bias table with one-tile windows on an unpadded grid: the tiled kernels, with or without the matrix-core scratch (the
    # scratch layout has no room for the streaming kernels' table-gradient partials at these shapes)
    out += [("bf16", 8, 4, 2, 2, 64, "table", True), ("bf16", 14, 7, 3, 2, 64, "table", True), ("f32", 8, 4, 2, 2, 32, "table", False)]
    return out


def onehot_cases():
    """(dtype, R, w, shift, H, C, perm): 2 hd codes must cover the window (n <= 64 at hd 32, n <= 32 at hd 16)"""
    out = []
    for (dn, R, w, s, H, C) in small_cases():
        if w * w <= 2 * (C // H):
            out += [(dn, R, w, s, H, C, perm) for perm in (0, 1)]
    return out


def region_cases():
    return [(dn, R, w, s, H, C) for (dn, R, w, s, H, C) in small_cases() if s > 0 and w in (4, 8)]


# the zero-bias fixture in table form, where the region sizes are powers of two (w = 4): EVERY (query, key) pair of a region
# contributes to d(bias table), so a single lost contribution shows; padded grid (tiled and streaming kernels) and one-tile windows
REGION_TABLE = [("bf16", 9, 4, 2, 2, 64, True), ("bf16", 9, 4, 2, 2, 64, False), ("f32", 9, 4, 2, 2, 32, False), ("bf16", 9, 4, 2, 2, 32, False),
                ("bf16", 8, 4, 2, 2, 64, True), ("f32", 8, 4, 2, 2, 64, False)]
