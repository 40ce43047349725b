"""Thin torch-tensor wrappers over the C ABI (one Python function per entry point of klab_mm.h).

Used by the parity tests and by host-side orchestration; tensors only provide device memory
(`data_ptr()`) and the current HIP stream -- the arithmetic is in libklab_mm.so.
"""
import ctypes as C

import torch

from . import _lib as L


def _seed_ptr(seed):
    return None if seed is None else seed.data_ptr()


def _gemm_args(A, B, C_out, *, M, N, K, a_kmajor=True, b_kmajor=True, lda=None, ldb=None, ldc=None, alpha=1.0,
               alpha_dev=None, bias=None, act=L.ACT_NONE, aux=None, aux_mode=L.AUX_NONE, aux_scale=1.0, residual=None,
               drop_p=0.0, seed=None, tag=0, accumulate=False, atomic_ok=False, name_tag=0):
    a = L.GemmArgs()
    a.atomic_ok, a.name_tag = int(atomic_ok), name_tag
    a.M, a.N, a.K = M, N, K
    a.dtype = L.dtype_code(A.dtype)
    assert B.dtype == A.dtype
    a.A, a.lda, a.a_kmajor = A.data_ptr(), (lda if lda is not None else A.stride(0)), int(a_kmajor)
    a.B, a.ldb, a.b_kmajor = B.data_ptr(), (ldb if ldb is not None else B.stride(0)), int(b_kmajor)
    a.C, a.ldc, a.c_dtype = C_out.data_ptr(), (ldc if ldc is not None else C_out.stride(0)), L.dtype_code(C_out.dtype)
    a.accumulate = int(accumulate)
    a.alpha = alpha
    a.alpha_dev = L.ptr(alpha_dev)
    a.bias = L.ptr(bias)
    a.act = act
    a.aux, a.ldaux, a.aux_mode, a.aux_scale = L.ptr(aux), (aux.stride(0) if aux is not None else 0), aux_mode, aux_scale
    a.residual = L.ptr(residual)
    a.ldr = residual.stride(0) if residual is not None else 0
    a.r_dtype = L.dtype_code(residual.dtype) if residual is not None else 0
    a.drop_p, a.seed_dev, a.drop_tag = drop_p, _seed_ptr(seed), tag
    return a


def gemm(A, B, C_out, **kw):
    """C_out = epilogue(alpha * A B^T): the keywords are the fields of klab_gemm_args (see _gemm_args)"""
    lib = L.load()
    a = _gemm_args(A, B, C_out, **kw)
    L.check(lib.klab_gemm(C.byref(a), L.stream_ptr()), "klab_gemm")
    return C_out


def gemm_grouped(members, large_tiles=False):
    """n independent GEMMs in one call (klab_gemm_grouped_tiles): `members` is a list of dicts, each holding the operands A, B, C and
    the keywords of `gemm`.  large_tiles: ask for the 256 x 256 grouped kernel (the whole list falls back to the 128-wide grouping
    when a member does not have its form, or when there are more than 32 members)."""
    lib = L.load()
    arr = (L.GemmArgs * max(len(members), 1))()
    for i, m in enumerate(members):
        kw = dict(m)
        arr[i] = _gemm_args(kw.pop("A"), kw.pop("B"), kw.pop("C"), **kw)
    L.check(lib.klab_gemm_grouped_tiles(C.cast(arr, C.c_void_p), len(members), int(bool(large_tiles)), L.stream_ptr()),
            "klab_gemm_grouped_tiles")


def quant_fp8_rows(x):
    """bf16 [M, K] -> (uint8 e4m3 [M, K], f32 row scales [M])"""
    import torch
    lib = L.load()
    M, K = x.shape
    x8 = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    sc = torch.empty(M, dtype=torch.float32, device=x.device)
    L.check(lib.klab_quant_fp8_rows(x.data_ptr(), x.stride(0), M, K, x8.data_ptr(), x8.stride(0), sc.data_ptr(), L.stream_ptr()),
            "klab_quant_fp8_rows")
    return x8, sc


def gemm_fp8(A8, sa, B8, sb, C_out, *, alpha=1.0, bias=None, act=L.ACT_NONE, residual=None, drop_p=0.0, seed=None, tag=0, name_tag=0):
    """C[M,N] = epilogue(alpha * sa[m] sb[n] * A8 @ B8^T): A8 [M,K], B8 [N,K] e4m3 bytes (uint8), per-row scales"""
    lib = L.load()
    a = L.GemmArgs()
    a.M, a.K = A8.shape
    a.N = B8.shape[0]
    a.dtype = L.BF16
    a.name_tag = name_tag  # 2: the block-scaled kernel (mmf8.hip) when K % 128 == 0, 3: never
    a.A, a.lda, a.a_kmajor = A8.data_ptr(), A8.stride(0), 1
    a.B, a.ldb, a.b_kmajor = B8.data_ptr(), B8.stride(0), 1
    a.C, a.ldc, a.c_dtype = C_out.data_ptr(), C_out.stride(0), L.dtype_code(C_out.dtype)
    a.alpha = alpha
    a.bias = L.ptr(bias)
    a.act = act
    a.residual = L.ptr(residual)
    a.ldr = residual.stride(0) if residual is not None else 0
    a.r_dtype = L.dtype_code(residual.dtype) if residual is not None else 0
    a.drop_p, a.seed_dev, a.drop_tag = drop_p, _seed_ptr(seed), tag
    L.check(lib.klab_gemm_fp8(C.byref(a), sa.data_ptr(), sb.data_ptr(), 1, L.stream_ptr()), "klab_gemm_fp8")
    return C_out


def rmsnorm_fwd(x, w, y=None, y_f32=None, rstd=None, eps=1e-6, grp=0, grp_stride=0, off=0, drop_p=0.0, seed=None, tag=0):
    lib = L.load()
    rows, d = x.shape
    L.check(lib.klab_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), L.ptr(y), L.dtype_code(y.dtype) if y is not None else 0,
                                 L.ptr(y_f32), L.ptr(rstd), rows, d, eps, grp, grp_stride, off, drop_p, _seed_ptr(seed), tag,
                                 L.stream_ptr()), "klab_rmsnorm_fwd")


def rmsnorm_bwd(dy, x, w, rstd, dres=None, dx=None, dxt=None, dw=None, grp=0, grp_stride=0, off=0, p_y=0.0, tag_y=0,
                p_prev=0.0, tag_prev=0, seed=None):
    lib = L.load()
    rows, d = x.shape
    L.check(lib.klab_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), L.ptr(dres), L.ptr(dx), L.ptr(dxt),
                                 L.dtype_code(dxt.dtype) if dxt is not None else 0, L.ptr(dw), rows, d, grp, grp_stride, off,
                                 p_y, tag_y, p_prev, tag_prev, _seed_ptr(seed), L.stream_ptr()), "klab_rmsnorm_bwd")


def rmsnorm_part_rows(rows):
    """rows of the partial-sum buffer klab_rmsnorm_bwd_part writes for `rows` input rows"""
    return int(L.load().klab_rmsnorm_part_rows(int(rows)))


def rmsnorm_bwd_part(dy, x, w, rstd, dw_part, dres=None, dx=None, dxt=None, grp=0, grp_stride=0, off=0, p_y=0.0, tag_y=0,
                     p_prev=0.0, tag_prev=0, seed=None):
    """rmsnorm_bwd with the weight gradient left as per-workgroup partial sums: dw_part [rmsnorm_part_rows(rows), d] is overwritten"""
    lib = L.load()
    rows, d = x.shape
    L.check(lib.klab_rmsnorm_bwd_part(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), L.ptr(dres), L.ptr(dx), L.ptr(dxt),
                                      L.dtype_code(dxt.dtype) if dxt is not None else 0, dw_part.data_ptr(), rows, d, grp, grp_stride,
                                      off, p_y, tag_y, p_prev, tag_prev, _seed_ptr(seed), L.stream_ptr()), "klab_rmsnorm_bwd_part")


def colpart_reduce(part, call_stride, nparts, d, dsts):
    """dsts[c][:d] += sum_b part[c * call_stride + b * d + :d] for b < nparts: `part` is a flat f32 buffer, `dsts` a list of f32
    vectors (one per call)"""
    lib = L.load()
    table = torch.tensor([t.data_ptr() for t in dsts], dtype=torch.int64).to(part.device)
    L.check(lib.klab_colpart_reduce(part.data_ptr(), int(call_stride), int(nparts), int(d), table.data_ptr(), len(dsts), L.stream_ptr()),
            "klab_colpart_reduce")
    return table  # (read by the kernel already enqueued: the caching allocator keeps its memory ordered behind the stream)


def layernorm_fwd(y, gamma, beta, shortcut=None, out=None, outt=None, mean=None, rstd=None, eps=1e-5, grp=0, grp_stride=0,
                  off=0, drop_p=0.0, seed=None, tag=0):
    lib = L.load()
    rows, Cc = y.shape
    L.check(lib.klab_layernorm_fwd(y.data_ptr(), L.dtype_code(y.dtype), gamma.data_ptr(), beta.data_ptr(), L.ptr(shortcut),
                                   L.ptr(out), L.ptr(outt), L.dtype_code(outt.dtype) if outt is not None else 0, L.ptr(mean),
                                   L.ptr(rstd), rows, Cc, eps, grp, grp_stride, off, drop_p, _seed_ptr(seed), tag,
                                   L.stream_ptr()), "klab_layernorm_fwd")


def swin_qkv_attn_fused(x, wqkv, bqkv, ctx, bias, logit_scale, *, B, R, w, shift, H, C):
    """ctx = window attention of (x @ wqkv.T + bqkv) without materialising q|k|v (frozen Swin-V2, HF/swinv2:389-455)."""
    lib = L.load()
    L.check(lib.klab_swin_qkv_attn_fused(x.data_ptr(), wqkv.data_ptr(), L.ptr(bqkv), ctx.data_ptr(), bias.data_ptr(), logit_scale.data_ptr(),
                                         L.dtype_code(x.dtype), B, R, w, shift, H, C, L.stream_ptr()), "klab_swin_qkv_attn_fused")


def swin_bias_image(bias, *, R, w, shift):
    """Dense bias [H, n, n] (swin_cpb_bias) -> the image [classes, H, 4, 64, 16] swin_qkv_attn_fused_img reads: bias + shift mask (-200) +
    key padding (-inf) in the score MFMA's lane order; classes = 4 with a shift (last window row x last window column), else 1."""
    import torch
    lib = L.load()
    H = bias.shape[0]
    nbytes = lib.klab_swin_bias_image_bytes(w, shift, H)
    if nbytes == 0:
        raise NotImplementedError("klab: unsupported shape/alignment in klab_swin_bias_image_bytes")
    image = torch.empty(nbytes // (H * 4 * 64 * 16 * 4), H, 4, 64, 16, device=bias.device, dtype=torch.float32)
    L.check(lib.klab_swin_bias_image(bias.data_ptr(), image.data_ptr(), R, w, shift, H, L.stream_ptr()), "klab_swin_bias_image")
    return image


def swin_qkv_attn_fused_img(x, wqkv, bqkv, ctx, image, logit_scale, *, B, R, w, shift, H, C):
    """swin_qkv_attn_fused on the pre-arranged image of swin_bias_image(bias, R=R, w=w, shift=shift): the same ctx, bit for bit."""
    lib = L.load()
    L.check(lib.klab_swin_qkv_attn_fused_img(x.data_ptr(), wqkv.data_ptr(), L.ptr(bqkv), ctx.data_ptr(), image.data_ptr(),
                                             logit_scale.data_ptr(), L.dtype_code(x.dtype), B, R, w, shift, H, C, L.stream_ptr()),
            "klab_swin_qkv_attn_fused_img")


def swin_proj_ln_fused(x, shortcut, w, b, gamma, beta, out, outt=None, eps=1e-5):
    """out = shortcut + LN(x @ w.T + b)*gamma+beta (frozen Swin-V2 attention-output half, C in {64,128})."""
    lib = L.load()
    M, Cc = x.shape
    L.check(lib.klab_swin_proj_ln_fused(x.data_ptr(), shortcut.data_ptr(), w.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                        out.data_ptr(), L.ptr(outt), L.dtype_code(x.dtype), M, Cc, eps, L.stream_ptr()), "klab_swin_proj_ln_fused")


def swin_mlp_fused(x, shortcut, w1, b1, w2, b2, gamma, beta, out, outt=None, eps=1e-5):
    """out = shortcut + LN(fc2(GELU(fc1(x)+b1))+b2)*gamma+beta (frozen Swin-V2 MLP half, C in {64,128}); raises
    NotImplementedError for other widths (HF/swinv2:539-563, 697-702)."""
    lib = L.load()
    M, Cc = x.shape
    L.check(lib.klab_swin_mlp_fused(x.data_ptr(), shortcut.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                    gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), L.ptr(outt), L.dtype_code(x.dtype), M, Cc, eps,
                                    L.stream_ptr()), "klab_swin_mlp_fused")


def rmsnorm_fwd_q8(x, w, y, rstd, y8, yscale, eps=1e-6, drop_p=0.0, seed=None, tag=0):
    """fp8 mode: y (bf16) = dropout(RMS-norm(x) * w) and the same rows in e4m3 (y8 uint8 [rows, d]) with one scale per row"""
    lib = L.load()
    rows, d = x.shape
    L.check(lib.klab_rmsnorm_fwd_q8(x.data_ptr(), w.data_ptr(), y.data_ptr(), L.ptr(rstd), y8.data_ptr(), yscale.data_ptr(), rows, d, eps,
                                    drop_p, _seed_ptr(seed), tag, L.stream_ptr()), "klab_rmsnorm_fwd_q8")


def layernorm_fwd_q8(y, gamma, beta, shortcut, out, outt, mean, rstd, o8, oscale, eps=1e-5):
    """fp8 mode: klab_layernorm_fwd with a bf16 `outt`, plus the same rows in e4m3 and one scale per row"""
    lib = L.load()
    rows, Cc = y.shape
    L.check(lib.klab_layernorm_fwd_q8(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), L.ptr(shortcut), L.ptr(out), outt.data_ptr(), L.ptr(mean),
                                      L.ptr(rstd), o8.data_ptr(), oscale.data_ptr(), rows, Cc, eps, L.stream_ptr()), "klab_layernorm_fwd_q8")


def gelu_fwd(z, a):
    """a = gelu(z), elementwise (the trainable Swin tower keeps the pre-activation z for the backward)"""
    lib = L.load()
    L.check(lib.klab_gelu_fwd(z.data_ptr(), a.data_ptr(), L.dtype_code(z.dtype), z.numel(), L.stream_ptr()), "klab_gelu_fwd")


def geglu_fwd(ab, h, drop_p=0.0, seed_dev=None, tag=0):
    """gate of the T5 v1.1 feed-forward: h [M, F] = dropout(gelu_new(ab[:, :F]) * ab[:, F:]); ab [M, 2F] (row stride free)"""
    lib = L.load()
    M, F = h.shape
    assert ab.shape == (M, 2 * F) and ab.dtype == h.dtype and ab.stride(1) == 1 and h.stride(1) == 1
    L.check(lib.klab_geglu_fwd(ab.data_ptr(), ab.stride(0), h.data_ptr(), h.stride(0), L.dtype_code(h.dtype), M, F, float(drop_p),
                               L.ptr(seed_dev), int(tag), L.stream_ptr()), "klab_geglu_fwd")


def geglu_bwd(dh, ab, dab, drop_p=0.0, seed_dev=None, tag=0):
    """dab [M, 2F] = (d a | d b) of geglu_fwd from dh [M, F] and the pre-activations ab [M, 2F]; the mask is regenerated from (seed, tag)"""
    lib = L.load()
    M, F = dh.shape
    assert ab.shape == (M, 2 * F) and dab.shape == (M, 2 * F) and ab.dtype == dh.dtype == dab.dtype
    assert ab.stride(1) == 1 and dh.stride(1) == 1 and dab.stride(1) == 1
    L.check(lib.klab_geglu_bwd(dh.data_ptr(), dh.stride(0), ab.data_ptr(), ab.stride(0), dab.data_ptr(), dab.stride(0),
                               L.dtype_code(dh.dtype), M, F, float(drop_p), L.ptr(seed_dev), int(tag), L.stream_ptr()), "klab_geglu_bwd")


def gelu_fwd_q8(z, a, a8, ascale):
    lib = L.load()
    rows, F = z.shape
    L.check(lib.klab_gelu_fwd_q8(z.data_ptr(), a.data_ptr(), a8.data_ptr(), ascale.data_ptr(), rows, F, L.stream_ptr()), "klab_gelu_fwd_q8")


def layernorm_bwd(dout, y, gamma, mean, rstd, dy=None, dgamma=None, dbeta=None, grp=0, grp_stride=0, off=0, drop_p=0.0,
                  seed=None, tag=0, dprev_bias=None):
    lib = L.load()
    rows, Cc = y.shape
    if dprev_bias is not None:
        L.check(lib.klab_layernorm_bwd_bias(dout.data_ptr(), y.data_ptr(), L.dtype_code(y.dtype), gamma.data_ptr(), mean.data_ptr(),
                                            rstd.data_ptr(), L.ptr(dy), L.ptr(dgamma), L.ptr(dbeta), dprev_bias.data_ptr(), rows, Cc, grp,
                                            grp_stride, off, drop_p, _seed_ptr(seed), tag, L.stream_ptr()), "klab_layernorm_bwd_bias")
        return
    L.check(lib.klab_layernorm_bwd(dout.data_ptr(), y.data_ptr(), L.dtype_code(y.dtype), gamma.data_ptr(), mean.data_ptr(),
                                   rstd.data_ptr(), L.ptr(dy), L.ptr(dgamma), L.ptr(dbeta), rows, Cc, grp, grp_stride, off,
                                   drop_p, _seed_ptr(seed), tag, L.stream_ptr()), "klab_layernorm_bwd")


def _attn_args(q, k, v, ctx, lse, bias, causal, B, H, Lq, Lk, dk, drop_p, seed, tag, ldq, ldk, ldv, ldo):
    a = L.AttnArgs()
    a.dtype = L.dtype_code(q.dtype)
    a.q, a.ldq = q.data_ptr(), ldq
    a.k, a.ldk = k.data_ptr(), ldk
    a.v, a.ldv = v.data_ptr(), ldv
    a.bias, a.causal = L.ptr(bias), int(causal)
    a.ctx, a.ldo, a.lse = ctx.data_ptr(), ldo, L.ptr(lse)
    a.B, a.H, a.Lq, a.Lk, a.dk = B, H, Lq, Lk, dk
    a.drop_p, a.seed_dev, a.drop_tag = drop_p, _seed_ptr(seed), tag
    return a


def t5_attn_fwd(q, k, v, ctx, lse, *, B, H, Lq, Lk, dk, bias=None, causal=False, drop_p=0.0, seed=None, tag=0,
                ldq=None, ldk=None, ldv=None, ldo=None):
    lib = L.load()
    a = _attn_args(q, k, v, ctx, lse, bias, causal, B, H, Lq, Lk, dk, drop_p, seed, tag,
                   ldq or q.stride(0), ldk or k.stride(0), ldv or v.stride(0), ldo or ctx.stride(0))
    L.check(lib.klab_t5_attn_fwd(C.byref(a), L.stream_ptr()), "klab_t5_attn_fwd")


def swin_linear_ln_fused(x, shortcut, w, bias, gamma, beta, out, outt=None, *, eps=1e-5):
    """shortcut + LayerNorm(x @ w.T + bias) * gamma + beta in one launch (klab_swin_linear_ln_fused); NotImplementedError outside the
    envelope (bf16, 256 output columns, K a multiple of 64)"""
    lib = L.load()
    M, K = x.shape
    L.check(lib.klab_swin_linear_ln_fused(x.data_ptr(), shortcut.data_ptr(), w.data_ptr(), bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                          out.data_ptr(), L.ptr(outt), L.dtype_code(x.dtype), M, K, w.shape[0], eps, L.stream_ptr()),
            "klab_swin_linear_ln_fused")


def swin_patch_embed_fused(pixels, w_padded, bias, gamma, beta, out, outt, *, patch=4, eps=1e-5):
    """LayerNorm(Conv2d(3 -> C, k 4, s 4)(pixels)) in one launch (klab_swin_patch_embed_fused); w_padded: bf16 [C, 64], columns 48.. zero"""
    lib = L.load()
    B, cin, H, _ = pixels.shape
    L.check(lib.klab_swin_patch_embed_fused(pixels.data_ptr(), w_padded.data_ptr(), w_padded.stride(0), bias.data_ptr(), gamma.data_ptr(),
                                            beta.data_ptr(), out.data_ptr(), L.ptr(outt), L.dtype_code(w_padded.dtype), B, cin, H, patch,
                                            out.shape[1], eps, L.stream_ptr()), "klab_swin_patch_embed_fused")


def t5_attn_fused_fwd(x, gamma, w, xn, rstd, proj, ctx, lse, *, B, H, Lq, Lk, dk, eps=1e-6, bias=None, causal=False, cross=False, k=None, v=None,
                      ldk=None, ldv=None, drop_p=0.0, seed=None, tag=0):
    """T5LayerNorm -> q|k|v (self) / q (cross) projection -> attention in one launch (klab_t5_attn_fused_fwd); NotImplementedError
    outside the envelope (bf16, d_model 512, head dim 64, at most 64 queries / keys)"""
    lib = L.load()
    fa = L.AttnFusedArgs()
    fa.x, fa.gamma, fa.eps, fa.d_model = x.data_ptr(), gamma.data_ptr(), eps, x.shape[1]
    fa.w, fa.xn, fa.rstd, fa.proj, fa.ldproj, fa.cross = w.data_ptr(), xn.data_ptr(), rstd.data_ptr(), proj.data_ptr(), proj.stride(0), int(cross)
    kk, vv = (k, v) if cross else (proj, proj)
    fa.attn = _attn_args(proj, kk, vv, ctx, lse, bias, causal, B, H, Lq, Lk, dk, drop_p, seed, tag, proj.stride(0),
                         ldk or kk.stride(0), ldv or vv.stride(0), ctx.stride(0))
    L.check(lib.klab_t5_attn_fused_fwd(C.byref(fa), L.stream_ptr()), "klab_t5_attn_fused_fwd")


def t5_attn_bwd(q, k, v, ctx, lse, dctx, dq, dk_out, dv, *, B, H, Lq, Lk, dk, bias=None, causal=False, dbias=None,
                drop_p=0.0, seed=None, tag=0, ldq=None, ldk=None, ldv=None, ldo=None, lddo=None, lddq=None, lddk=None,
                lddv=None, ds_ws=None, ds_defer=False):
    lib = L.load()
    a = _attn_args(q, k, v, ctx, lse, bias, causal, B, H, Lq, Lk, dk, drop_p, seed, tag,
                   ldq or q.stride(0), ldk or k.stride(0), ldv or v.stride(0), ldo or ctx.stride(0))
    a.dctx, a.lddo = dctx.data_ptr(), lddo or dctx.stride(0)
    a.dq, a.lddq = dq.data_ptr(), lddq or dq.stride(0)
    a.dk_out, a.lddk = dk_out.data_ptr(), lddk or dk_out.stride(0)
    a.dv, a.lddv = dv.data_ptr(), lddv or dv.stride(0)
    a.dbias = L.ptr(dbias)
    a.ds_ws, a.ds_defer = L.ptr(ds_ws), int(ds_defer)
    L.check(lib.klab_t5_attn_bwd(C.byref(a), L.stream_ptr()), "klab_t5_attn_bwd")


def t5_attn_bwd_fused(dy, w, q, k, v, ctx, lse, dq, dk_out, dv, *, B, H, Lq, Lk, dk, bias=None, causal=False, dbias=None, ds_ws=None,
                      ds_defer=False, drop_p=0.0, seed=None, tag=0, ldq=None, ldk=None, ldv=None, ldo=None, lddq=None, lddk=None, lddv=None):
    """o / co projection dgrad (dy @ w, kept on chip) -> attention backward in one launch (klab_t5_attn_bwd_fused); NotImplementedError
    outside the envelope (bf16, d_model 512, head dim 64, H * dk = 512, at most 64 queries / keys)"""
    lib = L.load()
    fb = L.AttnBwdFusedArgs()
    fb.dy, fb.lddy, fb.w, fb.d_model = dy.data_ptr(), dy.stride(0), w.data_ptr(), dy.shape[1]
    a = _attn_args(q, k, v, ctx, lse, bias, causal, B, H, Lq, Lk, dk, drop_p, seed, tag,
                   ldq or q.stride(0), ldk or k.stride(0), ldv or v.stride(0), ldo or ctx.stride(0))
    a.dq, a.lddq = dq.data_ptr(), lddq or dq.stride(0)
    a.dk_out, a.lddk = dk_out.data_ptr(), lddk or dk_out.stride(0)
    a.dv, a.lddv = dv.data_ptr(), lddv or dv.stride(0)
    a.dbias, a.ds_ws, a.ds_defer = L.ptr(dbias), L.ptr(ds_ws), int(ds_defer)
    fb.attn = a
    L.check(lib.klab_t5_attn_bwd_fused(C.byref(fb), L.stream_ptr()), "klab_t5_attn_bwd_fused")


def dbias_reduce(ds_ws, dbias, *, nbatch, H, Lq, Lk):
    """dbias [H, Lq, Lk] += sum of the nbatch stored-dS slabs ds_ws [nbatch, H, Lq, roundup(Lk, 32)] (bf16)"""
    lib = L.load()
    L.check(lib.klab_dbias_reduce(ds_ws.data_ptr(), L.dtype_code(ds_ws.dtype), dbias.data_ptr(), nbatch, H, Lq, Lk, L.stream_ptr()),
            "klab_dbias_reduce")


def decode_attn_map(q, k, out, *, R, H, Lk, dk, q_bstride, kv_bstride, ldk, out_bstride, q_div=1, kv_group=1, bias_row=None, bias_ld=0,
                    done=None):
    """out[r*out_bstride + j] (f32) = the head mean of softmax_j(q_h . k_{h,j} + bias_row[h, j]) for the one query row of each of
    R decoding rows: row r's query at q + (r // q_div)*q_bstride, its keys in sample r // kv_group at k + s*kv_bstride + j*ldk,
    head h at column h*dk (element strides; q and k bf16 or f32, the same).  bias_row f32 [H, bias_ld] or None; done int32 [R] or
    None: rows with done[r] != 0 get zeros.  V is not read (klab_t5_decode_attn_map, csrc/attn_map.hip)."""
    lib = L.load()
    if k.dtype != q.dtype or out.dtype != torch.float32:
        raise ValueError("decode_attn_map: q and k share a dtype and the map is float32")
    L.check(lib.klab_t5_decode_attn_map(L.dtype_code(q.dtype), q.data_ptr(), q_bstride, q_div, k.data_ptr(), kv_bstride, ldk, kv_group,
                                        L.ptr(bias_row), bias_ld, L.ptr(done), out.data_ptr(), out_bstride, R, H, Lk, dk, L.stream_ptr()),
            "klab_t5_decode_attn_map")


def decode_attn(q, k, v, ctx, *, R, H, Lk, dk, q_bstride, kv_bstride, ldk, ctx_bstride, kv_group=1, kv_slot=None, slot_ld=0,
                bias_row=None, bias_ld=0):
    """ctx[r*ctx_bstride + h*dk + c] = sum_j softmax_j(q_h . k_{h,j} + bias_row[h, j]) v_{h,j,c} (unscaled scores) for the one query
    row of each of R decoding rows: row r's query at q + r*q_bstride; key j of row r at k + s*kv_bstride + j*ldk with
    s = kv_slot[r*slot_ld + j] (int32 [R, slot_ld]) or, without a table, s = r // kv_group; v likewise; head h at column h*dk
    (element strides; q, k, v and ctx bf16 or f32, the same).  bias_row f32 [H, bias_ld] or None.  q, k, v may be views into one
    cache: only their data pointers are used (klab_t5_beam_decode_attn, csrc/attn_t5.hip)."""
    if q is None or k is None or v is None or ctx is None:
        raise ValueError("decode_attn: q, k, v and ctx are required")
    if not (q.dtype == k.dtype == v.dtype == ctx.dtype) or q.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("decode_attn: q, k, v and ctx share one dtype, bf16 or f32")
    if R <= 0 or H <= 0 or Lk <= 0 or kv_group < 1:
        raise ValueError("decode_attn: R, H, Lk and kv_group are positive")
    if kv_slot is not None and (kv_slot.dtype != torch.int32 or slot_ld < Lk):
        raise ValueError("decode_attn: kv_slot is int32 with a pitch of at least Lk")
    if bias_row is not None and (bias_row.dtype != torch.float32 or bias_ld < Lk):
        raise ValueError("decode_attn: bias_row is float32 with a pitch of at least Lk")
    if dk not in (8, 16, 32, 64, 128):
        raise NotImplementedError(f"decode_attn: head dim {dk} (8, 16, 32, 64 or 128)")
    lib = L.load()
    L.check(lib.klab_t5_beam_decode_attn(L.dtype_code(q.dtype), q.data_ptr(), q_bstride, k.data_ptr(), v.data_ptr(), kv_bstride, ldk,
                                         kv_group, L.ptr(kv_slot), slot_ld, L.ptr(bias_row), bias_ld, ctx.data_ptr(), ctx_bstride, R, H, Lk,
                                         dk, L.stream_ptr()), "klab_t5_beam_decode_attn")


def _swin_args(qkv, ctx, bias, logit_scale, lse, B, R, w, shift, H, Cc, bias_table=None, v_bias=None, dv_bias=None):
    a = L.SwinAttnArgs()
    a.v_bias, a.dv_bias = L.ptr(v_bias), L.ptr(dv_bias)
    a.dtype = L.dtype_code(qkv.dtype)
    a.qkv, a.ctx, a.bias, a.logit_scale, a.lse = qkv.data_ptr(), ctx.data_ptr(), L.ptr(bias), logit_scale.data_ptr(), L.ptr(lse)
    a.bias_table = L.ptr(bias_table)
    a.B, a.R, a.w, a.shift, a.H, a.C = B, R, w, shift, H, Cc
    return a


def swin_attn_fwd(qkv, ctx, bias, logit_scale, lse=None, *, B, R, w, shift, H, C, bias_table=None, mfma=True, v_bias=None):
    """bias [H, n, n] dense, or bias=None + bias_table [(2w-1)^2, H] (large windows: looked up per score); mfma=True hands the
    kernel the scratch its matrix-core form needs for windows of more than 64 tokens (False: the vector-ALU tiled kernel)"""
    import torch
    lib = L.load()
    a = _swin_args(qkv, ctx, bias, logit_scale, lse, B, R, w, shift, H, C, bias_table, v_bias)
    if mfma and (w * w > 64 or R % w):
        nbytes = lib.klab_swin_attn_bwd_ws_bytes(a.dtype, B, R, w, H, C)
        if nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=qkv.device)
            a.bwd_ws, a.bwd_ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.klab_swin_attn_fwd(C_byref(a), L.stream_ptr()), "klab_swin_attn_fwd")


def swin_attn_bwd(qkv, ctx, bias, logit_scale, lse, dctx, dqkv, dbias=None, dlogit_scale=None, *, B, R, w, shift, H, C, mfma=True,
                  bias_table=None, dbias_table=None, v_bias=None, dv_bias=None):
    """mfma=True hands the kernel its scratch (when the shape is inside the matrix-core envelope); False forces the VALU form.
    dqkv is overwritten; dbias, dbias_table, dlogit_scale and dv_bias are ACCUMULATED into (the caller clears them)."""
    import torch
    lib = L.load()
    a = _swin_args(qkv, ctx, bias, logit_scale, lse, B, R, w, shift, H, C, bias_table, v_bias, dv_bias)
    a.dbias_table = L.ptr(dbias_table)
    a.dctx, a.dqkv, a.dbias, a.dlogit_scale = dctx.data_ptr(), dqkv.data_ptr(), L.ptr(dbias), L.ptr(dlogit_scale)
    nbytes = lib.klab_swin_attn_bwd_ws_bytes(a.dtype, B, R, w, H, C) if mfma else 0
    if nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=qkv.device)
        a.bwd_ws, a.bwd_ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.klab_swin_attn_bwd(C_byref(a), L.stream_ptr()), "klab_swin_attn_bwd")


C_byref = C.byref


def swin_cpb_bias(coords, index, w0, b0, w2, table, bias, hidden=None, *, n, heads):
    lib = L.load()
    L.check(lib.klab_swin_cpb_bias(coords.data_ptr(), index.data_ptr(), w0.data_ptr(), b0.data_ptr(), w2.data_ptr(),
                                   table.data_ptr(), L.ptr(hidden), bias.data_ptr(), coords.shape[0], n, heads, w0.shape[0],
                                   L.stream_ptr()), "klab_swin_cpb_bias")


def swin_cpb_table(coords, w0, b0, w2, table, bias_table, hidden=None, *, heads):
    lib = L.load()
    L.check(lib.klab_swin_cpb_table(coords.data_ptr(), w0.data_ptr(), b0.data_ptr(), w2.data_ptr(), table.data_ptr(), L.ptr(hidden),
                                    bias_table.data_ptr(), coords.shape[0], heads, w0.shape[0], L.stream_ptr()), "klab_swin_cpb_table")


def swin_cpb_table_bwd(dbias_table, bias_table, coords, hidden, w2, dtable, dw0, db0, dw2, *, heads):
    lib = L.load()
    L.check(lib.klab_swin_cpb_table_bwd(dbias_table.data_ptr(), bias_table.data_ptr(), coords.data_ptr(), hidden.data_ptr(), w2.data_ptr(),
                                        dtable.data_ptr(), dw0.data_ptr(), db0.data_ptr(), dw2.data_ptr(), coords.shape[0], heads,
                                        hidden.shape[1], L.stream_ptr()), "klab_swin_cpb_table_bwd")


def swin_cpb_bias_bwd(dbias, bias, index, coords, hidden, w2, dtable, dw0, db0, dw2, *, heads, n=None, ntab=None, nhidden=None,
                      dtable_zeroed=False, w0=None):
    """backward of swin_cpb_bias from the dense dbias [H, n*n]: dtable [ntab, H] is scratch and result (cleared here unless
    dtable_zeroed says the caller did; the scatter then adds to whatever it holds), dw0 [nh, 2], db0 [nh] and dw2 [H, nh] are
    ACCUMULATED into.  n, ntab and nhidden default to what index, coords and hidden say (klab_swin_cpb_bias_bwd_pz; w0 is unused by
    the gradient and may stay None)."""
    lib = L.load()
    ntab = coords.shape[0] if ntab is None else ntab
    nhidden = hidden.shape[1] if nhidden is None else nhidden
    n = int(round(index.numel() ** 0.5)) if n is None else n
    L.check(lib.klab_swin_cpb_bias_bwd_pz(dbias.data_ptr(), bias.data_ptr(), index.data_ptr(), coords.data_ptr(), hidden.data_ptr(),
                                          L.ptr(w0), w2.data_ptr(), dtable.data_ptr(), dw0.data_ptr(), db0.data_ptr(), dw2.data_ptr(),
                                          ntab, n, heads, nhidden, 1 if dtable_zeroed else 0, L.stream_ptr()),
            "klab_swin_cpb_bias_bwd_pz")


def ce_fwd(logits, labels, inv_n, loss_row, loss, write_grad=True):
    lib = L.load()
    rows, V = logits.shape
    L.check(lib.klab_ce_fwd(logits.data_ptr(), logits.stride(0), L.dtype_code(logits.dtype), labels.data_ptr(), rows, V,
                            inv_n.data_ptr(), loss_row.data_ptr(), loss.data_ptr(), int(write_grad), L.stream_ptr()), "klab_ce_fwd")


def ce_count(labels, inv_n):
    """inv_n[0] = 1 / (number of labels != -100), 0 when there is none"""
    lib = L.load()
    L.check(lib.klab_ce_count(labels.data_ptr(), labels.numel(), inv_n.data_ptr(), L.stream_ptr()), "klab_ce_count")


def ce_wsum(labels, weights, inv_w):
    """inv_w[0] = 1 / (sum of weights[i] over the labels != -100), 0 when that sum is 0; weights None = all ones"""
    lib = L.load()
    L.check(lib.klab_ce_wsum(labels.data_ptr(), L.ptr(weights), labels.numel(), inv_w.data_ptr(), L.stream_ptr()), "klab_ce_wsum")


def ce_fwd_opts(logits, labels, weights, inv_w, loss_row, loss, *, eps=0.0, z=0.0, write_grad=True):
    """ce_fwd with label smoothing eps, z-loss z and per-row weights (f32 [rows] or None); loss_row gets the unweighted row losses"""
    lib = L.load()
    rows, V = logits.shape
    L.check(lib.klab_ce_fwd_opts(logits.data_ptr(), logits.stride(0), L.dtype_code(logits.dtype), labels.data_ptr(), L.ptr(weights), rows, V,
                                 float(eps), float(z), inv_w.data_ptr(), loss_row.data_ptr(), loss.data_ptr(), int(write_grad),
                                 L.stream_ptr()), "klab_ce_fwd_opts")


def ce_fwd_distill(logits, teacher, labels, weights, inv_w, loss_row, kl_row, loss, *, eps=0.0, z=0.0, alpha=0.5, temperature=1.0,
                   write_grad=True):
    """ce_fwd_opts mixed with the KL divergence from `teacher` ([rows, V] bf16 or f32 logits, only read, finite) at `temperature`:
    l = (1 - alpha) ce + alpha T^2 kl; loss_row gets the unweighted l, kl_row the unweighted kl"""
    lib = L.load()
    rows, V = logits.shape
    L.check(lib.klab_ce_fwd_distill(logits.data_ptr(), logits.stride(0), L.dtype_code(logits.dtype), teacher.data_ptr(), teacher.stride(0),
                                    L.dtype_code(teacher.dtype), labels.data_ptr(), L.ptr(weights), rows, V, float(eps), float(z), float(alpha),
                                    float(temperature), inv_w.data_ptr(), loss_row.data_ptr(), kl_row.data_ptr(), loss.data_ptr(),
                                    int(write_grad), L.stream_ptr()), "klab_ce_fwd_distill")


def ciderd_rewards(hyp, refs, keys, idf, log_n, out, *, n_h=1, sigma=6.0, eos=1, count_eos=True):
    """out[r] (f32 [rows]) = CIDEr-D over token ids of row r of hyp (int64 [rows, L], start token first) against the present
    references of image r // n_h in refs (int64 [B, R, Lr], label format); (keys, idf): the document-frequency table
    (int64-viewed uint64 keys and f32 values, a power of two of slots), log_n the weight of an n-gram it does not hold"""
    lib = L.load()
    rows, Lh = hyp.shape
    B, R, Lr = refs.shape
    if rows != B * n_h:
        raise ValueError(f"hyp holds {rows} rows, refs {B} images of {n_h} hypotheses")
    L.check(lib.klab_ciderd_rewards(hyp.data_ptr(), rows, int(n_h), Lh, refs.data_ptr(), R, Lr, keys.data_ptr(), idf.data_ptr(), keys.numel(),
                                    float(log_n), float(sigma), int(eos), int(bool(count_eos)), out.data_ptr(), L.stream_ptr()),
            "klab_ciderd_rewards")


def scst_targets(seq, rewards, baseline, labels, weights, advantages, *, n, mode, eos=1):
    """labels / weights [rows, Lt] and advantages [rows] of the sequences seq (int64 [rows, L], rows = B * n) under rewards
    (f32 [rows]); mode 0: minus baseline (f32 [B]), 1: leave-one-out over the image's n rows, 2: no baseline"""
    lib = L.load()
    rows, Ls = seq.shape
    L.check(lib.klab_scst_targets(seq.data_ptr(), rows, int(n), Ls, rewards.data_ptr(), L.ptr(baseline), int(mode), int(eos),
                                  labels.shape[-1], labels.data_ptr(), weights.data_ptr(), advantages.data_ptr(), L.stream_ptr()),
            "klab_scst_targets")


def caption_stats(hyp, refs, stats, *, n_h=1, eos=1, count_eos=False):
    """stats (int32 [rows, 16]) = BLEU-1..4 / ROUGE-L sufficient statistics of row r of hyp (int64 [rows, L], start token first)
    against the present references of image r // n_h in refs (int64 [B, R, Lr], label format); columns as in include/klab_mm.h"""
    lib = L.load()
    rows, Lh = hyp.shape
    B, R, Lr = refs.shape
    if rows != B * n_h or stats.numel() != rows * 16:
        raise ValueError(f"hyp holds {rows} rows, refs {B} images of {n_h} hypotheses, stats {stats.numel()} elements")
    L.check(lib.klab_caption_stats(hyp.data_ptr(), rows, int(n_h), Lh, refs.data_ptr(), R, Lr, int(eos), int(bool(count_eos)),
                                   stats.data_ptr(), L.stream_ptr()), "klab_caption_stats")


def embed_fwd(ids, table, out, *, shift_right=False, L_seq=1, start_id=0, pad_id=0, drop_p=0.0, seed=None, tag=0, err=None):
    lib = L.load()
    rows, d = out.shape
    L.check(lib.klab_embed_fwd(ids.data_ptr(), int(shift_right), L_seq, start_id, pad_id, table.data_ptr(), table.shape[0],
                               out.data_ptr(), rows, d, drop_p, _seed_ptr(seed), tag, L.ptr(err), L.stream_ptr()), "klab_embed_fwd")


def embed_bwd(ids, dh, dtable, *, shift_right=False, L_seq=1, start_id=0, pad_id=0, drop_p=0.0, seed=None, tag=0):
    lib = L.load()
    rows, d = dh.shape
    L.check(lib.klab_embed_bwd(ids.data_ptr(), int(shift_right), L_seq, start_id, pad_id, dh.data_ptr(), dtable.data_ptr(),
                               dtable.shape[0], rows, d, drop_p, _seed_ptr(seed), tag, L.stream_ptr()), "klab_embed_bwd")


def relbias_fwd(table, bucket, bias):
    lib = L.load()
    H, Lq, Lk = bias.shape
    L.check(lib.klab_relbias_fwd(table.data_ptr(), bucket.data_ptr(), bias.data_ptr(), H, Lq, Lk, L.stream_ptr()), "klab_relbias_fwd")


def relbias_bwd(dbias, bucket, dtable):
    lib = L.load()
    H, Lq, Lk = dbias.shape
    L.check(lib.klab_relbias_bwd(dbias.data_ptr(), bucket.data_ptr(), dtable.data_ptr(), H, Lq, Lk, dtable.shape[0],
                                 L.stream_ptr()), "klab_relbias_bwd")


def im2col_patch(pixels, out, P):
    lib = L.load()
    B, Cin, Himg, _ = pixels.shape
    ldo = out.shape[-1]
    if ldo == Cin * P * P:
        L.check(lib.klab_im2col_patch(pixels.data_ptr(), out.data_ptr(), L.dtype_code(out.dtype), B, Cin, Himg, P, L.stream_ptr()),
                "klab_im2col_patch")
    else:  # padded rows: tail columns are zero-filled
        L.check(lib.klab_im2col_patch_ld(pixels.data_ptr(), out.data_ptr(), L.dtype_code(out.dtype), B, Cin, Himg, P, ldo, L.stream_ptr()),
                "klab_im2col_patch_ld")


def merge_gather(x, out, *, B, R, C):
    lib = L.load()
    L.check(lib.klab_merge_gather(x.data_ptr(), out.data_ptr(), L.dtype_code(out.dtype), B, R, C, L.stream_ptr()), "klab_merge_gather")


def merge_scatter(dm, dx, *, B, R, C):
    lib = L.load()
    L.check(lib.klab_merge_scatter(dm.data_ptr(), dx.data_ptr(), B, R, C, L.stream_ptr()), "klab_merge_scatter")


def colsum(dy, out):
    lib = L.load()
    M, N = dy.shape
    L.check(lib.klab_colsum(dy.data_ptr(), dy.stride(0), L.dtype_code(dy.dtype), M, N, out.data_ptr(), L.stream_ptr()), "klab_colsum")


def convert(x, y, scale=1.0):
    lib = L.load()
    L.check(lib.klab_convert(x.data_ptr(), y.data_ptr(), L.dtype_code(y.dtype), x.numel(), scale, L.stream_ptr()), "klab_convert")


def add_f32(y, x):
    """y += x, both f32 with a length that is a multiple of 4"""
    lib = L.load()
    assert y.dtype == x.dtype == torch.float32 and y.numel() == x.numel()
    L.check(lib.klab_add_f32(y.data_ptr(), x.data_ptr(), y.numel(), L.stream_ptr()), "klab_add_f32")


# ---- descriptor-table kernels: `desc` is an int64 device tensor [n, fields] in the struct layout of the kernel's table ----------
def cast_pack(desc, total4, dst):
    """multi-tensor f32 -> dst.dtype cast into the flat buffer `dst`; desc [n, 3] rows of CastDesc {src pointer, dst_off (elements),
    n4_prefix (exclusive prefix sum of the tensors' lengths / 4)}, total4 the sum of all lengths / 4"""
    lib = L.load()
    assert desc.dtype == torch.int64 and desc.dim() == 2 and desc.shape[1] == 3 and desc.is_contiguous()
    L.check(lib.klab_cast_pack(desc.data_ptr(), desc.shape[0], int(total4), dst.data_ptr(), L.dtype_code(dst.dtype), L.stream_ptr()),
            "klab_cast_pack")


def quant_fp8_arena(desc, total_rows, arena_bf16, arena_fp8, scales):
    """every row of the listed tensors of a bf16 arena -> e4m3 bytes at the same element offsets of arena_fp8 (uint8), the row's scale at
    scales[(off + r*K) / 8]; desc [n, 4] rows of QuantDesc {off, rows, K, row0 (exclusive prefix sum of rows)}"""
    lib = L.load()
    assert desc.dtype == torch.int64 and desc.dim() == 2 and desc.shape[1] == 4 and desc.is_contiguous()
    L.check(lib.klab_quant_fp8_arena(desc.data_ptr(), desc.shape[0], int(total_rows), arena_bf16.data_ptr(), arena_fp8.data_ptr(),
                                     scales.data_ptr(), L.stream_ptr()), "klab_quant_fp8_arena")


def adam_step(desc, total4, grads, m, v, arena, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, bias_corr1=1.0, bias_corr2=1.0,
              begin4=None, end4=None):
    """one torch.optim.Adam update of every tensor of the table (klab_adam_step), or of the vec4 range [begin4, end4) of its prefix
    space (klab_adam_step_range); desc [n, 4] rows of AdamDesc {p pointer, goff (element offset into grads / m / v), aoff (element
    offset of the compute-dtype copy in `arena`, < 0: none), n4_prefix}, total4 the sum of all lengths / 4"""
    lib = L.load()
    assert desc.dtype == torch.int64 and desc.dim() == 2 and desc.shape[1] == 4 and desc.is_contiguous()
    hyper = (float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), float(bias_corr1), float(bias_corr2))
    if begin4 is None and end4 is None:
        L.check(lib.klab_adam_step(desc.data_ptr(), desc.shape[0], int(total4), grads.data_ptr(), m.data_ptr(), v.data_ptr(),
                                   arena.data_ptr(), L.dtype_code(arena.dtype), *hyper, L.stream_ptr()), "klab_adam_step")
    else:
        L.check(lib.klab_adam_step_range(desc.data_ptr(), desc.shape[0], int(begin4), int(end4), grads.data_ptr(), m.data_ptr(),
                                         v.data_ptr(), arena.data_ptr(), L.dtype_code(arena.dtype), *hyper, L.stream_ptr()),
                "klab_adam_step_range")


def adamw_step(desc, group_of, groups, grads, m, v, arena, *, begin4=0, end4=None, total4=None):
    """one torch.optim.AdamW update (decoupled decay) of the vec4 range [begin4, end4) of the table's prefix space in ONE launch,
    whatever the number of parameter groups (klab_adamw_step_range).  desc as for adam_step; group_of: int32 device tensor [n], the
    group of each tensor in table order; groups: 1 .. 16 dicts (or tuples) of lr, beta1, beta2, eps, weight_decay, bias_corr1,
    bias_corr2 -- host values, passed to the kernel by value.  end4 defaults to total4 (the whole table)."""
    lib = L.load()
    assert desc.dtype == torch.int64 and desc.dim() == 2 and desc.shape[1] == 4 and desc.is_contiguous()
    assert group_of.dtype == torch.int32 and group_of.is_contiguous() and group_of.numel() == desc.shape[0] and group_of.device == desc.device
    end4 = total4 if end4 is None else end4
    L.check(lib.klab_adamw_step_range(desc.data_ptr(), desc.shape[0], group_of.data_ptr(), L.adamw_groups(groups), len(groups), int(begin4),
                                      int(end4), grads.data_ptr(), m.data_ptr(), v.data_ptr(), arena.data_ptr(), L.dtype_code(arena.dtype),
                                      L.stream_ptr()), "klab_adamw_step_range")


def ema_update(desc, ema, w, *, begin4=0, end4=None, total4=None):
    """one EMA update e' = e + w (p - e) of the vec4 range [begin4, end4) of the table's prefix space in ONE launch
    (klab_ema_update_range).  desc as for adam_step; ema: fp32 device tensor laid out like grads / m / v (indexed by goff); w: host
    float in [0, 1], passed to the kernel by value.  The parameters are only read.  end4 defaults to total4 (the whole table)."""
    lib = L.load()
    assert desc.dtype == torch.int64 and desc.dim() == 2 and desc.shape[1] == 4 and desc.is_contiguous()
    assert ema.dtype == torch.float32 and ema.is_contiguous()
    end4 = total4 if end4 is None else end4
    L.check(lib.klab_ema_update_range(desc.data_ptr(), desc.shape[0], int(begin4), int(end4), ema.data_ptr(), float(w), L.stream_ptr()),
            "klab_ema_update_range")


def ema_swap(desc, ema, arena, *, begin4=0, end4=None, total4=None):
    """exchange the bits of every parameter of the vec4 range [begin4, end4) with its slice of `ema` and write the compute-dtype
    copy of the new parameter into `arena` (bf16 or fp32; tensors with aoff < 0 have none) in ONE launch (klab_ema_swap_range).
    Two calls restore both bit for bit.  end4 defaults to total4 (the whole table)."""
    lib = L.load()
    assert desc.dtype == torch.int64 and desc.dim() == 2 and desc.shape[1] == 4 and desc.is_contiguous()
    assert ema.dtype == torch.float32 and ema.is_contiguous()
    end4 = total4 if end4 is None else end4
    L.check(lib.klab_ema_swap_range(desc.data_ptr(), desc.shape[0], int(begin4), int(end4), ema.data_ptr(), arena.data_ptr(),
                                    L.dtype_code(arena.dtype), L.stream_ptr()), "klab_ema_swap_range")


def lora_row_block():
    """rows of a target matrix one workgroup of the LoRA kernels owns (a compile-time constant of the library; no GPU needed)"""
    return int(L.load().klab_lora_row_block())


def lora_plan(shapes, row_block=None):
    """host side of the LoRA table for targets of shapes [(out, in, r)]: per tensor (n4_prefix, rb_prefix, slab_off, db_off) and the
    element counts (out_elems, slab_elems) of the two fp32 buffers klab_lora_grads writes -- dA of tensor t at out[4 * n4_prefix], dB
    at out[db_off], its partials [row blocks, r, in] at slab[slab_off]"""
    rb = lora_row_block() if row_block is None else int(row_block)
    n4 = blocks = slab = 0
    rows = []
    for out, inn, r in shapes:
        out, inn, r = int(out), int(inn), int(r)
        if out < 1 or inn < 4 or inn % 4 or not 1 <= r <= 64:
            raise ValueError(f"klab: LoRA target [{out}, {inn}] with r = {r}: needs in % 4 == 0 and 1 <= r <= 64")
        nb = (out + rb - 1) // rb
        rows.append([n4, blocks, slab, 0])
        n4 += r * inn // 4
        blocks += nb
        slab += nb * r * inn
    db = 4 * n4
    for row, (out, _inn, r) in zip(rows, shapes):
        row[3] = db
        db += (int(out) * int(r) + 3) & ~3
    return [tuple(r) for r in rows], db, slab


def lora_table(entries):
    """the device table of lora_merge / lora_grads: entries = [(W [out, in], A [r, in], B [out, r], arena_off, grad_off, s)], fp32
    contiguous tensors of one device; returns (desc int64 [n, 11], plan rows, out_elems, slab_elems) as lora_plan gives them"""
    import struct
    shapes = []
    for W, A, B, aoff, goff, _s in entries:
        for t in (W, A, B):
            if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda or t.data_ptr() % 16:
                raise ValueError("klab: LoRA tensors have to be contiguous 16-byte aligned fp32 device tensors")
        if W.dim() != 2 or tuple(A.shape) != (A.shape[0], W.shape[1]) or tuple(B.shape) != (W.shape[0], A.shape[0]):
            raise ValueError(f"klab: LoRA shapes W {tuple(W.shape)}, A {tuple(A.shape)}, B {tuple(B.shape)} do not fit")
        if int(aoff) % 4 or int(goff) % 4:
            raise ValueError("klab: arena and gradient offsets have to be multiples of 4 elements")
        shapes.append((W.shape[0], W.shape[1], A.shape[0]))
    plan, out_elems, slab_elems = lora_plan(shapes)
    rows = []
    for (W, A, B, aoff, goff, s), (out, inn, r), (n4, rbp, so, db) in zip(entries, shapes, plan):
        sbits = struct.unpack("<I", struct.pack("<f", float(s)))[0]
        rs = (sbits << 32) | r
        rows.append([W.data_ptr(), A.data_ptr(), B.data_ptr(), int(aoff), int(goff), (inn << 32) | out, rs - (1 << 64) if rs >= 1 << 63 else rs,
                     n4, rbp, so, db])
    dev = entries[0][0].device if entries else "cuda"
    host = torch.tensor(rows, dtype=torch.int64).reshape(-1, 11).pin_memory()  # pinned: the upload does not synchronise
    return host.to(dev, non_blocking=True), plan, out_elems, slab_elems


def lora_merge(desc, arena=None, to_master=False):
    """arena[arena_off + i * in + j] = cast(W[i,j] + s sum_k B[i,k] A[k,j]) for every tensor of the table in ONE launch
    (klab_lora_merge; arena bf16 or fp32); to_master=True: the same fp32 value into W itself, no arena"""
    lib = L.load()
    assert desc.dtype == torch.int64 and desc.dim() == 2 and desc.shape[1] == 11 and desc.is_contiguous()
    if not to_master and (arena is None or arena.dtype not in (torch.float32, torch.bfloat16)):
        raise ValueError("klab: lora_merge needs a bf16 or fp32 arena (or to_master=True)")
    L.check(lib.klab_lora_merge(desc.data_ptr(), desc.shape[0], None if to_master else arena.data_ptr(),
                                0 if to_master else L.dtype_code(arena.dtype), int(bool(to_master)), L.stream_ptr()), "klab_lora_merge")


def lora_grads(desc, grads, out, slab):
    """dB = s dW A^T and dA = s B^T dW of every tensor of the table from the flat gradient buffer `grads`, in two launches
    (klab_lora_grads); out, slab: fp32 device buffers of at least lora_plan's out_elems / slab_elems.  Both outputs are overwritten."""
    lib = L.load()
    assert desc.dtype == torch.int64 and desc.dim() == 2 and desc.shape[1] == 11 and desc.is_contiguous()
    assert grads.dtype == out.dtype == slab.dtype == torch.float32 and out.is_contiguous() and slab.is_contiguous()
    L.check(lib.klab_lora_grads(desc.data_ptr(), desc.shape[0], grads.data_ptr(), out.data_ptr(), slab.data_ptr(), L.stream_ptr()),
            "klab_lora_grads")


def grad_norm_chunk():
    """elements per fp64 partial of grad_norm (a compile-time constant of the library; no GPU needed)"""
    return int(L.load().klab_grad_norm_chunk())


def grad_norm_plan(numels, chunk=None):
    """host side of the gradient table: tensor i of `numels` owns partials [first[i], first[i] + ceil(numels[i] / chunk));
    returns (first, nparts)"""
    chunk = grad_norm_chunk() if chunk is None else int(chunk)
    first, run = [], 0
    for n in numels:
        n = int(n)
        if n < 1:
            raise ValueError("klab: a gradient tensor of the table has no elements")
        first.append(run)
        run += (n + chunk - 1) // chunk
    return first, run


def grad_table(tensors):
    """the device table of grad_norm / grad_clip for fp32 contiguous tensors of one device: desc int64 [n, 2] rows of
    {pointer, numel}; returns (desc, nparts)"""
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda for t in tensors)
    _first, nparts = grad_norm_plan([t.numel() for t in tensors])
    rows = [[t.data_ptr(), t.numel()] for t in tensors]
    dev = tensors[0].device if tensors else "cuda"
    host = torch.tensor(rows, dtype=torch.int64).reshape(-1, 2).pin_memory()  # pinned: the upload does not synchronise
    return host.to(dev, non_blocking=True), nparts


def grad_norm(desc, parts, norms, kind=0, nparts=None):
    """norms[i] = the L2 norm (kind 0) or max |g| (kind 1) of tensor i of the table, norms[n] = that of all of them (klab_grad_norm);
    parts: float64 scratch of at least `nparts` elements (grad_table's count; checked when given), norms: float32 [>= n + 1]"""
    lib = L.load()
    assert desc.dtype == torch.int64 and desc.dim() == 2 and desc.shape[1] == 2 and desc.is_contiguous()
    assert parts.dtype == torch.float64 and norms.dtype == torch.float32 and norms.numel() >= desc.shape[0] + 1
    if nparts is not None and parts.numel() < nparts:
        raise ValueError(f"klab: grad_norm needs {nparts} partials, the buffer holds {parts.numel()}")
    L.check(lib.klab_grad_norm(desc.data_ptr(), desc.shape[0], int(kind), parts.data_ptr(), parts.numel(), norms.data_ptr(), L.stream_ptr()),
            "klab_grad_norm")


def grad_clip(desc, total, max_norm, coef):
    """coef[0] = min(max_norm / (total[0] + 1e-6), 1) (NaN kept) and every tensor of the table times coef in place, or no store at
    all when coef >= 1 (klab_grad_clip); total, coef: float32 device tensors of one element, e.g. views of grad_norm's `norms`"""
    lib = L.load()
    assert desc.dtype == torch.int64 and desc.dim() == 2 and desc.shape[1] == 2 and desc.is_contiguous()
    assert total.dtype == coef.dtype == torch.float32
    L.check(lib.klab_grad_clip(desc.data_ptr(), desc.shape[0], total.data_ptr(), float(max_norm), coef.data_ptr(), L.stream_ptr()),
            "klab_grad_clip")


def image_preprocess(src_u8, desc, n, max_h, max_w, pixel_values, *, mid=256, out=224, filter_a=3, filter_b=2,
                     rescale=1.0 / 255 / 255, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
    """klab_image_preprocess: src_u8 device uint8 bytes, desc device int64 [n, 2] rows of {offset, height | width << 32}
    (the klab_image_desc layout), or filter_a=0 with src_u8 = [n, mid, mid, 3]."""
    import torch
    lib = L.load()
    m3 = (C.c_float * 3)(*mean)
    s3 = (C.c_float * 3)(*std)
    ws, nbytes = None, 0
    if filter_a:
        nbytes = lib.klab_image_preprocess_ws_bytes(n, max_h, mid)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=src_u8.device)
    L.check(lib.klab_image_preprocess(src_u8.data_ptr(), L.ptr(desc), n, max_h, max_w, mid, out, filter_a, filter_b, rescale,
                                      C.cast(m3, C.c_void_p), C.cast(s3, C.c_void_p), pixel_values.data_ptr(), L.ptr(ws), nbytes,
                                      L.stream_ptr()), "klab_image_preprocess")


IMAGE_FLIP_LR = 1  # KLAB_IMAGE_FLIP_LR


def image_crop_desc(offsets, sizes, boxes, flips):
    """host side of klab_image_crop_desc: int64 numpy [n, 3] rows of {offset, height | width << 32, pitch | flags << 32} for images
    of `sizes` (height, width) at byte `offsets`, cropped to `boxes` (top, left, h, w) and mirrored where `flips`.  `top` and `left`
    are folded into the offset; the boxes must have been checked against the sizes."""
    import numpy as np
    sz = np.asarray(sizes, np.int64).reshape(-1, 2)
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    fl = np.asarray(flips, bool).astype(np.int64) * IMAGE_FLIP_LR
    desc = np.empty((len(sz), 3), np.int64)
    desc[:, 0] = np.asarray(offsets, np.int64) + (b[:, 0] * sz[:, 1] + b[:, 1]) * 3
    desc[:, 1] = b[:, 2] | (b[:, 3] << 32)
    desc[:, 2] = sz[:, 1] | (fl << 32)
    return desc


def image_preprocess_crop(src_u8, desc, n, max_crop_h, max_crop_w, pixel_values, *, mid=256, out=224, filter_a=3, filter_b=2,
                          rescale=1.0 / 255 / 255, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
    """klab_image_preprocess_crop: image_preprocess on one sub-rectangle per image, mirrored where its flip bit is set.  desc:
    device int64 [n, 3] from image_crop_desc; max_crop_h / max_crop_w: the largest crop of the batch."""
    import torch
    lib = L.load()
    assert desc.dtype == torch.int64 and tuple(desc.shape) == (n, 3) and desc.is_contiguous()
    m3 = (C.c_float * 3)(*mean)
    s3 = (C.c_float * 3)(*std)
    nbytes = lib.klab_image_preprocess_ws_bytes(n, max_crop_h, mid)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=src_u8.device)
    L.check(lib.klab_image_preprocess_crop(src_u8.data_ptr(), desc.data_ptr(), n, max_crop_h, max_crop_w, mid, out, filter_a, filter_b,
                                           rescale, C.cast(m3, C.c_void_p), C.cast(s3, C.c_void_p), pixel_values.data_ptr(),
                                           ws.data_ptr(), nbytes, L.stream_ptr()), "klab_image_preprocess_crop")


# ---- JPEG (row f-1): host entropy decoding + device reconstruction ---------------------------------------------------------
def jpeg_read_info(data: bytes):
    """header of one JPEG file (host only): a _lib.JpegInfo"""
    lib = L.load()
    info = L.JpegInfo()
    data = data if isinstance(data, bytes) else bytes(data)
    L.check(lib.klab_jpeg_read_info(C.cast(C.c_char_p(data), C.c_void_p), len(data), C.byref(info)), "klab_jpeg_read_info")
    return info


def jpeg_entropy_decode_batch(datas, n_threads=8):
    """Huffman-decode a list of JPEG byte strings on the host (threaded).  Returns (coefs int16 numpy [total_blocks, 64] in pinned
    memory when CUDA is available, qt uint16 numpy [n, 3, 64], items = (_lib.JpegItem * n) with coef_block0 filled, rgb_off = byte
    offsets of 16-byte aligned HWC RGB images, total RGB bytes).  Unsupported files (CMYK, 12-bit, arithmetic-coded, ...) raise
    NotImplementedError naming the index."""
    import numpy as np
    import torch
    lib = L.load()
    n = len(datas)
    items = (L.JpegItem * n)()
    datas = [d if isinstance(d, bytes) else bytes(d) for d in datas]
    bufs = [C.c_char_p(d) for d in datas]  # pointers into the bytes objects (read-only use, `datas` outlives the calls)
    blocks, rgb = 0, 0
    for i, d in enumerate(datas):
        L.check(lib.klab_jpeg_read_info(C.cast(bufs[i], C.c_void_p), len(d), C.byref(items[i].info)), f"klab_jpeg_read_info[{i}]")
        f = items[i].info
        if not f.supported:
            raise NotImplementedError(f"klab: JPEG {i} is outside the device decoder (progressive={f.progressive}, components={f.ncomp}, "
                                      f"precision={f.precision}, sampling={list(f.hs)}x{list(f.vs)})")
        items[i].coef_block0 = blocks
        items[i].rgb_off = rgb
        blocks += f.coef_blocks
        rgb += (f.width * f.height * 3 + 15) // 16 * 16
    coefs_t = torch.empty((max(blocks, 1), 64), dtype=torch.int16, pin_memory=torch.cuda.is_available())
    coefs = coefs_t.numpy()
    qt = np.zeros((n, 3, 64), np.uint16)
    ptrs = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in bufs])
    sizes = (C.c_size_t * n)(*[len(d) for d in datas])
    cps = (C.c_void_p * n)(*[coefs.ctypes.data + items[i].coef_block0 * 128 for i in range(n)])
    infos = (L.JpegInfo * n)()
    rcs = (C.c_int * n)()
    rc = lib.klab_jpeg_entropy_decode_batch(C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), n, C.cast(cps, C.c_void_p),
                                            qt.ctypes.data, C.cast(infos, C.c_void_p), C.cast(rcs, C.c_void_p), int(n_threads))
    if rc:
        bad = [i for i in range(n) if rcs[i]]
        L.check(rcs[bad[0]] if bad else rc, f"klab_jpeg_entropy_decode_batch (images {bad})")
    return coefs_t, qt, items, rgb


def jpeg_decode_device(coefs_t, qt, items, rgb_bytes, device="cuda"):
    """device half: returns (rgb uint8 device buffer holding the HWC images at items[i].rgb_off, desc int64 [n, 2] device tensor in
    the klab_image_desc layout that image_preprocess takes)"""
    import numpy as np
    import torch
    lib = L.load()
    n = len(items)
    dev = torch.device(device)
    coefs_dev = coefs_t.to(dev, non_blocking=True)
    qt_dev = torch.from_numpy(qt.view(np.int16)).to(dev)
    raw = np.frombuffer(bytes(items), dtype=np.uint8).copy()
    items_dev = torch.from_numpy(raw).to(dev)
    nbytes = lib.klab_jpeg_decode_ws_bytes(C.cast(items, C.c_void_p), n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rgb = torch.empty(max(rgb_bytes, 16), dtype=torch.uint8, device=dev)
    L.check(lib.klab_jpeg_decode_device(coefs_dev.data_ptr(), qt_dev.data_ptr(), C.cast(items, C.c_void_p), items_dev.data_ptr(), n,
                                        rgb.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr()), "klab_jpeg_decode_device")
    desc = np.zeros((n, 2), np.int64)
    for i in range(n):
        desc[i, 0] = items[i].rgb_off
        desc[i, 1] = items[i].info.height | (items[i].info.width << 32)
    # (coefs_dev / qt_dev / items_dev / ws are consumed by kernels already enqueued on the current stream; the caching allocator
    # keeps their memory ordered behind that stream)
    return rgb, torch.from_numpy(desc).to(dev)


def jpeg_decode(datas, device="cuda", n_threads=8, pipelined=False):
    """list of JPEG byte strings -> list of HWC uint8 RGB device tensors (views into one buffer): `Image.open(f).convert('RGB')`"""
    if pipelined:
        rgb, _desc, items = jpeg_decode_pipelined(datas, device, n_threads)
    else:
        coefs_t, qt, items, rgb_bytes = jpeg_entropy_decode_batch(datas, n_threads)
        rgb, _desc = jpeg_decode_device(coefs_t, qt, items, rgb_bytes, device)
    out = []
    for it in items:
        h, w = it.info.height, it.info.width
        out.append(rgb[it.rgb_off:it.rgb_off + h * w * 3].view(h, w, 3))
    return out


def jpeg_decode_pipelined(datas, device="cuda", n_threads=8, n_chunks=4, on_headers=None):
    """file bytes -> (rgb device buffer, desc device tensor [n, 2] in the klab_image_desc layout, items).  The batch is cut into
    chunks: while the host threads Huffman-decode chunk i+1, chunk i's coefficients cross PCIe and are reconstructed on the GPU
    (the copies and kernels are asynchronous on the current stream; the host never waits for the device).  on_headers: called with
    the list of (height, width) once every header is read and before anything is allocated or enqueued (a caller's own checks)."""
    import numpy as np
    import torch
    lib = L.load()
    n = len(datas)
    dev = torch.device(device)
    datas = [d if isinstance(d, bytes) else bytes(d) for d in datas]
    items = (L.JpegItem * n)()
    blocks, rgb_bytes = 0, 0
    for i, d in enumerate(datas):
        L.check(lib.klab_jpeg_read_info(C.cast(C.c_char_p(d), C.c_void_p), len(d), C.byref(items[i].info)), f"klab_jpeg_read_info[{i}]")
        f = items[i].info
        if not f.supported:
            raise NotImplementedError(f"klab: JPEG {i} is outside the device decoder (components={f.ncomp}, precision={f.precision}, "
                                      f"sampling={list(f.hs)}x{list(f.vs)})")
        items[i].coef_block0, items[i].rgb_off = blocks, rgb_bytes
        blocks += f.coef_blocks
        rgb_bytes += (f.width * f.height * 3 + 15) // 16 * 16
    if on_headers is not None:
        on_headers([(it.info.height, it.info.width) for it in items])
    coefs_t = torch.empty((max(blocks, 1), 64), dtype=torch.int16, pin_memory=True)
    qt_t = torch.zeros((n, 192), dtype=torch.int16, pin_memory=True)
    coefs, qt = coefs_t.numpy(), qt_t.numpy()
    coefs_dev = torch.empty((max(blocks, 1), 64), dtype=torch.int16, device=dev)
    qt_dev = torch.empty((n, 192), dtype=torch.int16, device=dev)
    items_dev = torch.from_numpy(np.frombuffer(bytes(items), dtype=np.uint8).copy()).to(dev)
    rgb = torch.empty(max(rgb_bytes, 16), dtype=torch.uint8, device=dev)
    isz = C.sizeof(L.JpegItem)
    per = max(1, -(-n // max(1, n_chunks)))
    keep = []
    for lo in range(0, n, per):
        hi = min(n, lo + per)
        m = hi - lo
        ptrs = (C.c_void_p * m)(*[C.cast(C.c_char_p(datas[i]), C.c_void_p) for i in range(lo, hi)])
        sizes = (C.c_size_t * m)(*[len(datas[i]) for i in range(lo, hi)])
        cps = (C.c_void_p * m)(*[coefs.ctypes.data + items[i].coef_block0 * 128 for i in range(lo, hi)])
        rcs = (C.c_int * m)()
        rc = lib.klab_jpeg_entropy_decode_batch(C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), m, C.cast(cps, C.c_void_p),
                                                qt.ctypes.data + lo * 384, None, C.cast(rcs, C.c_void_p), int(n_threads))
        if rc:
            bad = [lo + i for i in range(m) if rcs[i]]
            L.check(rcs[bad[0] - lo] if bad else rc, f"klab_jpeg_entropy_decode_batch (images {bad})")
        b0 = items[lo].coef_block0
        b1 = items[hi - 1].coef_block0 + items[hi - 1].info.coef_blocks
        coefs_dev[b0:b1].copy_(coefs_t[b0:b1], non_blocking=True)
        qt_dev[lo:hi].copy_(qt_t[lo:hi], non_blocking=True)
        host_items = C.cast(C.addressof(items) + lo * isz, C.c_void_p)
        nbytes = lib.klab_jpeg_decode_ws_bytes(host_items, m)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        keep.append(ws)
        # qt index of image i in the kernel is (i - lo) * 3 + c: pass the chunk's slice of the table
        L.check(lib.klab_jpeg_decode_device(coefs_dev.data_ptr(), qt_dev.data_ptr() + lo * 384, host_items, items_dev.data_ptr() + lo * isz, m,
                                            rgb.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr()), "klab_jpeg_decode_device")
    desc = np.zeros((n, 2), np.int64)
    for i in range(n):
        desc[i, 0] = items[i].rgb_off
        desc[i, 1] = items[i].info.height | (items[i].info.width << 32)
    return rgb, torch.from_numpy(desc).to(dev), items
