"""Host-side handle on the native engine (klab_engine_* of include/klab_mm.h).

Builds the C config structs, mirrors the engine's parameter table (HuggingFace state-dict names),
computes the input-independent integer/float tables with the reference's own arithmetic
(T5 relative-position buckets HF/t5:216-262; Swin-V2 CPB coords/index HF/swinv2:457-492) and binds
caller-owned torch storage (parameters, flat gradient buffers, one workspace) to the plan.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import _lib as L


# ---- config mirrors (field names follow HF/swinv2cfg:56-73 and HF/t5cfg:44-62) -----------------
@dataclass
class SwinConfig:
    image_size: int = 224
    patch_size: int = 4
    num_channels: int = 3
    embed_dim: int = 96
    depths: Sequence[int] = (2, 2, 6, 2)
    num_heads: Sequence[int] = (3, 6, 12, 24)
    window_size: int = 7
    pretrained_window_sizes: Sequence[int] = (0, 0, 0, 0)
    mlp_ratio: float = 4.0
    qkv_bias: bool = True
    layer_norm_eps: float = 1e-5

    @classmethod
    def from_dict(cls, d):
        keys = cls.__dataclass_fields__.keys()
        c = cls(**{k: d[k] for k in keys if k in d and d[k] is not None})
        if isinstance(c.image_size, (list, tuple)):
            if c.image_size[0] != c.image_size[1]:
                raise NotImplementedError("non-square images are outside the scoped configs")
            c.image_size = c.image_size[0]
        if isinstance(c.patch_size, (list, tuple)):
            c.patch_size = c.patch_size[0]
        return c

    @property
    def hidden_size(self):
        return int(self.embed_dim * 2 ** (len(self.depths) - 1))


@dataclass
class T5Config:
    vocab_size: int = 32128
    d_model: int = 512
    d_kv: int = 64
    d_ff: int = 2048
    num_layers: int = 6
    num_decoder_layers: Optional[int] = None
    num_heads: int = 8
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    dropout_rate: float = 0.1
    layer_norm_epsilon: float = 1e-6
    feed_forward_proj: str = "relu"
    decoder_start_token_id: Optional[int] = 0
    pad_token_id: Optional[int] = 0
    eos_token_id: int = 1
    scale_decoder_outputs: bool = True
    tie_word_embeddings: bool = True  # False (T5 v1.1 / Flan-T5): lm_head.weight is a parameter of its own

    def __post_init__(self):
        if self.num_decoder_layers is None:
            self.num_decoder_layers = self.num_layers

    @classmethod
    def from_dict(cls, d):
        keys = cls.__dataclass_fields__.keys()
        c = cls(**{k: d[k] for k in keys if k in d and d[k] is not None})
        if "decoder_start_token_id" in d and d["decoder_start_token_id"] is None:
            c.decoder_start_token_id = None
        if d.get("tie_word_embeddings", None) is False:  # HF/t5cfg:82-83
            c.scale_decoder_outputs = False
            c.tie_word_embeddings = False
        return c


# ---- C structs -------------------------------------------------------------------------------
class CSwinCfg(C.Structure):
    _fields_ = [("image_size", C.c_int), ("patch", C.c_int), ("in_ch", C.c_int), ("embed_dim", C.c_int), ("n_stages", C.c_int),
                ("depths", C.c_int * 8), ("heads", C.c_int * 8), ("window", C.c_int), ("pretrained_window", C.c_int * 8),
                ("mlp_ratio", C.c_int), ("qkv_bias", C.c_int), ("ln_eps", C.c_float)]


class CT5Cfg(C.Structure):
    _fields_ = [("vocab", C.c_int), ("d_model", C.c_int), ("d_kv", C.c_int), ("n_heads", C.c_int), ("d_ff", C.c_int),
                ("n_layers", C.c_int), ("n_dec_layers", C.c_int), ("rel_buckets", C.c_int), ("rel_max_dist", C.c_int),
                ("dropout", C.c_float), ("ln_eps", C.c_float), ("start_id", C.c_int), ("pad_id", C.c_int),
                ("scale_decoder_outputs", C.c_int), ("ffn_gated", C.c_int), ("tie_lm_head", C.c_int)]


class CModelCfg(C.Structure):
    _fields_ = [("swin", CSwinCfg), ("lang", CT5Cfg), ("main", CT5Cfg), ("dtype", C.c_int), ("train_swin", C.c_int)]


ENGINE_SIGS = {
    "klab_engine_create": ([C.POINTER(CModelCfg)], C.c_void_p),
    "klab_engine_destroy": ([C.c_void_p], None),
    "klab_engine_num_params": ([C.c_void_p, C.c_int], C.c_int),
    "klab_engine_param_info": ([C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_int),
                                C.POINTER(C.c_long)], C.c_int),
    "klab_engine_grad_elems": ([C.c_void_p, C.c_int], C.c_long),
    "klab_engine_segment": ([C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_long)], C.c_int),
    "klab_engine_num_buckets": ([C.c_void_p, C.c_int], C.c_int),
    "klab_engine_bucket": ([C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long)], C.c_int),
    "klab_engine_bucket_wait": ([C.c_void_p, C.c_int, C.c_int, C.c_void_p], C.c_int),
    "klab_engine_set_bucket_events": ([C.c_void_p, C.c_int], C.c_int),
    "klab_engine_workspace_bytes": ([C.c_void_p, C.c_int, C.c_int, C.c_int], C.c_size_t),
    "klab_engine_workspace_bytes_n": ([C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int], C.c_size_t),
    "klab_engine_bind": ([C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                          C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                          C.POINTER(C.c_void_p), C.c_void_p], C.c_int),
    "klab_engine_forward": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_void_p], C.c_int),
    "klab_engine_gen_set_forced": ([C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p], C.c_int),
    "klab_engine_gen_attn_bytes": ([C.c_void_p, C.POINTER(L.GenCfg)], C.c_size_t),
    "klab_engine_gen_set_attn": ([C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p], C.c_int),
    "klab_engine_gen_set_constraint": ([C.c_void_p, C.POINTER(L.ConstraintCfg), C.c_void_p], C.c_int),
    "klab_engine_gen_workspace_bytes": ([C.c_void_p, C.POINTER(L.GenCfg)], C.c_size_t),
    "klab_engine_gen_begin": ([C.c_void_p, C.POINTER(L.GenCfg), C.c_void_p, C.c_void_p], C.c_int),
    "klab_engine_gen_step": ([C.c_void_p, C.c_int, C.c_void_p, C.c_void_p], C.c_int),
    "klab_engine_gen_stop_word": ([C.c_void_p, C.c_void_p, C.c_int], C.c_void_p),
    "klab_engine_gen_buffer": ([C.c_void_p, C.c_void_p, C.c_char_p, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_int)], C.c_void_p),
    "klab_engine_gen_result": ([C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "klab_engine_gen_scores": ([C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p], C.c_int),
    "klab_engine_backward": ([C.c_void_p, C.c_int, C.c_void_p, C.c_void_p], C.c_int),
    "klab_engine_set_graph": ([C.c_void_p, C.c_int], C.c_int),
    "klab_engine_get_rng": ([C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p], C.c_int),
    "klab_engine_set_rng": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p], C.c_int),
    "klab_engine_adam_step": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                               C.c_float, C.c_void_p], C.c_int),
    "klab_engine_adam_step_segment": ([C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                       C.c_float, C.c_float, C.c_void_p], C.c_int),
    "klab_engine_adam_layout": ([C.c_void_p, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_int)], C.c_int),
    "klab_engine_adamw_step": ([C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(L.AdamWGroup), C.c_int, C.c_void_p], C.c_int),
    "klab_engine_ema_update": ([C.c_void_p, C.c_void_p, C.c_float, C.c_void_p], C.c_int),
    "klab_engine_ema_swap": ([C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "klab_engine_lora_layout": ([C.c_void_p, C.c_int, C.POINTER(C.c_long)], C.c_int),
    "klab_engine_lora_set": ([C.c_void_p, C.c_void_p, C.c_int], C.c_int),
    "klab_engine_lora_grads": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "klab_engine_adafactor_state_elems": ([C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)], C.c_int),
    "klab_engine_adafactor_layout": ([C.c_void_p, C.c_int, C.POINTER(C.c_long)], C.c_int),
    "klab_engine_adafactor_step": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_float] * 9 + [C.c_int, C.c_void_p],
                                   C.c_int),
    "klab_engine_probe_enable": ([C.c_void_p, C.c_int], C.c_int),
    "klab_engine_probe_read": ([C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double)], C.c_int),
    "klab_engine_loss_ptr": ([C.c_void_p], C.c_void_p),
    "klab_engine_set_loss_out": ([C.c_void_p, C.c_void_p], C.c_int),
    "klab_engine_err_ptr": ([C.c_void_p], C.c_void_p),
    "klab_engine_rng_ptr": ([C.c_void_p], C.c_void_p),
    "klab_engine_buffer": ([C.c_void_p, C.c_char_p, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_int)], C.c_void_p),
    "klab_gelu_fwd": ([C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_void_p], C.c_int),
    "klab_sizeof_t5_cfg": ([], C.c_int),
    "klab_sizeof_model_cfg": ([], C.c_int),
    "klab_swin_cpb_bias_bwd": ([C.c_void_p] * 11 + [C.c_int] * 4 + [C.c_void_p], C.c_int),
    "klab_swin_cpb_bias_bwd_pz": ([C.c_void_p] * 11 + [C.c_int] * 5 + [C.c_void_p], C.c_int),
}
_sigs_installed = False


def lib():
    global _sigs_installed
    l = L.load()
    if not _sigs_installed:
        for name, (argt, rest) in ENGINE_SIGS.items():
            fn = getattr(l, name)
            fn.argtypes = argt
            fn.restype = rest
        _sigs_installed = True
    return l


FEED_FORWARD_PROJ = {"relu": 0, "gated-gelu": 1}  # HF/t5cfg feed_forward_proj -> klab_t5_cfg.ffn_gated


def _c_t5(c: T5Config) -> CT5Cfg:
    if c.feed_forward_proj not in FEED_FORWARD_PROJ:
        raise NotImplementedError(f"feed_forward_proj {c.feed_forward_proj!r}: only the v1.0 ReLU feed-forward ('relu') and the v1.1 / "
                                  "Flan-T5 gated gelu_new feed-forward ('gated-gelu') are implemented")
    if c.decoder_start_token_id is None:
        raise ValueError("self.model.config.decoder_start_token_id has to be defined.")  # HF/t5:622-626
    if c.pad_token_id is None:
        raise ValueError("self.model.config.pad_token_id has to be defined.")  # HF/t5:632-633
    return CT5Cfg(c.vocab_size, c.d_model, c.d_kv, c.num_heads, c.d_ff, c.num_layers, c.num_decoder_layers,
                  c.relative_attention_num_buckets, c.relative_attention_max_distance, float(c.dropout_rate),
                  float(c.layer_norm_epsilon), int(c.decoder_start_token_id), int(c.pad_token_id), int(c.scale_decoder_outputs),
                  FEED_FORWARD_PROJ[c.feed_forward_proj], int(c.tie_word_embeddings))


def _c_swin(c: SwinConfig) -> CSwinCfg:
    s = CSwinCfg()
    s.image_size, s.patch, s.in_ch, s.embed_dim, s.n_stages = c.image_size, c.patch_size, c.num_channels, c.embed_dim, len(c.depths)
    if len(c.depths) > 8:
        raise NotImplementedError("more than 8 Swin stages")
    for i, (dd, hh) in enumerate(zip(c.depths, c.num_heads)):
        s.depths[i], s.heads[i] = dd, hh
    for i, pw in enumerate(list(c.pretrained_window_sizes)[:len(c.depths)]):
        s.pretrained_window[i] = pw
    s.window = c.window_size
    if float(c.mlp_ratio) != int(c.mlp_ratio):
        raise NotImplementedError("fractional mlp_ratio")
    s.mlp_ratio, s.qkv_bias, s.ln_eps = int(c.mlp_ratio), int(c.qkv_bias), float(c.layer_norm_eps)
    return s


# ---- input-independent tables, computed with the reference's arithmetic ---------------------------
def t5_bucket_table(Lq: int, Lk: int, bidirectional: bool, num_buckets: int, max_distance: int) -> torch.Tensor:
    """T5Attention._relative_position_bucket over (memory - context) (HF/t5:216-262, 264-272).
    Kept in torch on the host so the float-log truncation is bit-identical to the reference's."""
    ctx = torch.arange(Lq, dtype=torch.long)[:, None]
    mem = torch.arange(Lk, dtype=torch.long)[None, :]
    rel = mem - ctx
    out = torch.zeros_like(rel)
    nb = num_buckets
    if bidirectional:
        nb //= 2
        out = out + (rel > 0).to(torch.long) * nb
        rel = torch.abs(rel)
    else:
        rel = -torch.min(rel, torch.zeros_like(rel))
    max_exact = nb // 2
    is_small = rel < max_exact
    large = max_exact + (torch.log(rel.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return (out + torch.where(is_small, rel, large)).to(torch.int32).contiguous()


def swin_cpb_tables(w: int, pretrained_w: int):
    """relative_coords_table [(2w-1)^2, 2] f32 and relative_position_index [w^2*w^2] i32 (HF/swinv2:457-492)."""
    rc = torch.arange(-(w - 1), w, dtype=torch.int64).float()
    table = torch.stack(torch.meshgrid([rc, rc], indexing="ij")).permute(1, 2, 0).contiguous().unsqueeze(0)
    if pretrained_w > 0:
        table = table / (pretrained_w - 1)
    elif w > 1:
        table = table / (w - 1)
    table = table * 8
    table = torch.sign(table) * torch.log2(torch.abs(table) + 1.0) / math.log2(8)
    c = torch.arange(w)
    coords = torch.stack(torch.meshgrid([c, c], indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += w - 1
    rel[:, :, 1] += w - 1
    rel[:, :, 0] *= 2 * w - 1
    return table.view(-1, 2).float().contiguous(), rel.sum(-1).view(-1).to(torch.int32).contiguous()


@dataclass
class ParamSpec:
    name: str
    shape: tuple
    grad_off: int


class Engine:
    """One native plan per (configs, dtype, train_swin).  bind() attaches storage for a batch shape."""

    MODELS = ("swin", "lang", "main")

    def __init__(self, swin: SwinConfig, lang: T5Config, main: T5Config, dtype=torch.bfloat16, train_swin=False):
        self.swin_cfg, self.lang_cfg, self.main_cfg = swin, lang, main
        self.dtype = dtype
        self.train_swin = bool(train_swin)
        if swin.hidden_size != main.d_model:
            # the reference fails at its torch.cat (ref/models/model.py:23) with this RuntimeError
            raise RuntimeError(f"Sizes of tensors must match except in dimension 1. Expected size {swin.hidden_size} "
                               f"but got size {main.d_model} for tensor number 1 in the list.")
        if lang.d_model != main.d_model:
            raise RuntimeError(f"Sizes of tensors must match except in dimension 1. Expected size {swin.hidden_size} "
                               f"but got size {lang.d_model} for tensor number 1 in the list.")
        if dtype == "fp8" and "gated-gelu" in (lang.feed_forward_proj, main.feed_forward_proj):
            raise NotImplementedError("dtype='fp8' with a gated-gelu feed-forward (T5 v1.1 / Flan-T5) is not implemented: use bf16")
        self._cfg = CModelCfg(_c_swin(swin), _c_t5(lang), _c_t5(main), L.dtype_code(dtype), int(self.train_swin))
        self._lib = lib()
        self._h = self._lib.klab_engine_create(C.byref(self._cfg))
        if not self._h:
            raise ValueError("klab_engine_create rejected the configuration")
        self.params = {m: self._param_table(i) for i, m in enumerate(self.MODELS)}
        self.grad_elems = {m: int(self._lib.klab_engine_grad_elems(self._h, i)) for i, m in enumerate(self.MODELS)}
        self.segments = []
        for s in range(3):
            mi, off, ln = C.c_int(), C.c_long(), C.c_long()
            L.check(self._lib.klab_engine_segment(self._h, s, C.byref(mi), C.byref(off), C.byref(ln)), "klab_engine_segment")
            self.segments.append((self.MODELS[mi.value], off.value, ln.value))
        self.buckets = []  # per segment: [(offset, length)] of the layer buckets, in the order backward finishes them
        for sg in range(3):
            out = []
            for i in range(max(0, self._lib.klab_engine_num_buckets(self._h, sg))):
                off, ln = C.c_long(), C.c_long()
                L.check(self._lib.klab_engine_bucket(self._h, sg, i, C.byref(off), C.byref(ln)), "klab_engine_bucket")
                out.append((off.value, ln.value))
            self.buckets.append(out)
        self._keep = None
        self.shape = None
        self._gen = None  # the klab_gen_cfg of the decoding session begun last
        self._forced = self._forced_armed = None  # forced-token tables: of that session / armed for the next gen_begin
        self._attn = self._attn_armed = None  # cross-attention maps, in the same two roles

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._lib.klab_engine_destroy(h)
            except Exception:
                pass

    def _param_table(self, mi) -> List[ParamSpec]:
        n = self._lib.klab_engine_num_params(self._h, mi)
        out = []
        buf = C.create_string_buffer(256)
        shape = (C.c_long * 4)()
        nd, go = C.c_int(), C.c_long()
        for i in range(n):
            L.check(self._lib.klab_engine_param_info(self._h, mi, i, buf, 256, shape, C.byref(nd), C.byref(go)), "param_info")
            out.append(ParamSpec(buf.value.decode(), tuple(shape[k] for k in range(nd.value)), go.value))
        return out

    def workspace_bytes(self, B, Ls, Lt, n=1) -> int:
        """bytes of a binding of B images with n captions each: a query, it changes nothing in the engine"""
        if int(n) < 1:
            raise ValueError(f"captions per image has to be >= 1, got {n}")
        return int(self._lib.klab_engine_workspace_bytes_n(self._h, B, Ls, Lt, int(n)))

    def bind(self, B, Ls, Lt, tensors, main_grads, swin_grads, device, n=1):
        """tensors: {model: [fp32 device tensors in table order]}.  n: captions per image -- the decoder side of the binding runs
        B*n target sequences in image-major order (tgt_ids [B, n, Lt]) over the B encoder outputs."""
        nbytes = self.workspace_bytes(B, Ls, Lt, n)
        if nbytes == 0:
            raise ValueError("bad batch shape")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        m = self.main_cfg
        lang_b = t5_bucket_table(Ls, Ls, True, self.lang_cfg.relative_attention_num_buckets,
                                 self.lang_cfg.relative_attention_max_distance).to(device)
        Le = self.n_img + Ls
        enc_b = t5_bucket_table(Le, Le, True, m.relative_attention_num_buckets, m.relative_attention_max_distance).to(device)
        dec_b = t5_bucket_table(Lt, Lt, False, m.relative_attention_num_buckets, m.relative_attention_max_distance).to(device)
        s = self.swin_cfg
        R0 = s.image_size // s.patch_size
        coords, index = [], []
        for st in range(len(s.depths)):
            R = R0 >> st
            w = min(R, s.window_size)
            pw = list(s.pretrained_window_sizes)[st] if st < len(s.pretrained_window_sizes) else 0
            ct, ix = swin_cpb_tables(w, pw)
            coords.append(ct.to(device))
            index.append(ix.to(device))
        arrs = {}
        for mname in self.MODELS:
            ts = tensors[mname]
            assert len(ts) == len(self.params[mname])
            for t, spec in zip(ts, self.params[mname]):
                if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != spec.shape or t.device != ws.device:
                    raise ValueError(f"parameter {mname}.{spec.name}: expected contiguous fp32 {spec.shape} on {ws.device}, "
                                     f"got {t.dtype} {tuple(t.shape)} on {t.device}")
            arrs[mname] = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        carr = (C.c_void_p * len(coords))(*[t.data_ptr() for t in coords])
        iarr = (C.c_void_p * len(index))(*[t.data_ptr() for t in index])
        L.check(self._lib.klab_engine_set_captions(self._h, int(n)), "klab_engine_set_captions")  # one-shot: this bind takes it
        rc = self._lib.klab_engine_bind(self._h, B, Ls, Lt, ws.data_ptr(), nbytes, arrs["swin"], arrs["lang"], arrs["main"],
                                        main_grads.data_ptr(), swin_grads.data_ptr() if swin_grads is not None else None,
                                        lang_b.data_ptr(), enc_b.data_ptr(), dec_b.data_ptr(), carr, iarr, L.stream_ptr())
        L.check(rc, "klab_engine_bind")
        self._keep = (ws, lang_b, enc_b, dec_b, coords, index, tensors, main_grads, swin_grads)
        self.shape = (B, Ls, Lt)
        self.captions = int(n)
        self.workspace = ws
        lp = self._lib.klab_engine_loss_ptr(self._h)
        off = lp - ws.data_ptr()
        self.loss_view = ws[off:off + 4].view(torch.float32)
        ep = self._lib.klab_engine_err_ptr(self._h)
        eo = ep - ws.data_ptr()
        self.err_view = ws[eo:eo + 4].view(torch.int32)
        ro = self._lib.klab_engine_rng_ptr(self._h) - ws.data_ptr()
        self.rng_view = ws[ro:ro + 12].view(torch.int32)  # {step seed, base seed, forwards since seeding}

    @property
    def n_img(self):
        s = self.swin_cfg
        Rl = (s.image_size // s.patch_size) >> (len(s.depths) - 1)
        return Rl * Rl

    def forward(self, pixels, src_ids, tgt_ids, training, seed, want_grad=True):
        L.check(self._lib.klab_engine_forward(self._h, pixels.data_ptr(), src_ids.data_ptr(), tgt_ids.data_ptr(), int(training),
                                              int(seed) & 0xFFFFFFFF, int(want_grad), L.stream_ptr()), "klab_engine_forward")

    def set_loss_out(self, out):
        """the next forward writes its loss into `out` (a 1-element fp32 device tensor) instead of loss_view; False under graph replay"""
        rc = self._lib.klab_engine_set_loss_out(self._h, out.data_ptr() if out is not None else None)
        if rc < 0:
            L.check(rc, "klab_engine_set_loss_out")
        return rc == 1

    def set_loss_options(self, eps=0.0, z=0.0, weights=None):
        """label smoothing and z-loss of the forwards from now on; `weights` (fp32 device tensor [B, Lt], [B, n, Lt] on a
        binding with n captions per image, or None) for the next forward only, which copies it (None disarms weights armed earlier)"""
        L.check(self._lib.klab_engine_set_loss_options(self._h, float(eps), float(z), weights.data_ptr() if weights is not None else None),
                "klab_engine_set_loss_options")

    def set_weight_norm(self, count=False):
        """normaliser of the weighted loss of the forwards from now on: the sum of the weights, or (count) the number of labels"""
        L.check(self._lib.klab_engine_set_weight_norm(self._h, 1 if count else 0), "klab_engine_set_weight_norm")

    def set_distill(self, alpha=0.0, temperature=1.0, teacher=None):
        """distillation weight and temperature of the forwards from now on; `teacher` (contiguous bf16 or fp32 device tensor of
        B*n*Lt x V logits, or None) for the next forward only, which reads it in place (None disarms a teacher armed earlier)"""
        code = L.dtype_code(teacher.dtype) if teacher is not None else L.dtype_code(torch.bfloat16)
        L.check(self._lib.klab_engine_set_distill(self._h, float(alpha), float(temperature), teacher.data_ptr() if teacher is not None else None,
                                                  code), "klab_engine_set_distill")

    # ---- decoding sessions (HF `_beam_search`, `_sample`, greedy decoding); the workspace is the caller's, the binding's is
    # untouched ----------------------------------------------------------------------------------------------------------------
    GEN_MODES = {"pick": L.GEN_PICK, "sample": L.GEN_SAMPLE, "beam": L.GEN_BEAM, "force": L.GEN_FORCE}
    EARLY_STOPPING = {False: 0, True: 1, "never": 2}

    @classmethod
    def gen_cfg(cls, mode, n, max_length, eos_id, pad_id, temperature=1.0, top_k=0, top_p=1.0, seed=0, length_penalty=1.0,
                early_stopping=False, procs=None, want_logprobs=False, constraint=None):
        """the klab_gen_cfg of a session; procs: the logits processors' settings (logits_proc.logits_processor_settings), None =
        none; want_logprobs: sampling and pick also keep every chosen token's log-probability (gen_scores); constraint: (trie,
        roots) -- a constrain.TokenTrie on the device and the int32 [B] device tensor of every image's start node -- None = none.
        klab_gen_cfg itself has no field for it: gen_workspace_bytes and gen_begin arm it (gen_set_constraint) for a cfg that
        carries one.  The cfg keeps the C arrays and tensors it points to alive."""
        cfg = L.GenCfg(cls.GEN_MODES[mode], int(n), int(max_length), int(eos_id), int(pad_id), float(temperature), int(top_k),
                       float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF, float(length_penalty), cls.EARLY_STOPPING[early_stopping])
        if procs is not None:
            words = [list(map(int, w)) for w in procs["bad_words_ids"]]
            off = [0]
            for w in words:
                off.append(off[-1] + len(w))
            toks = [t for w in words for t in w]
            off_a = (C.c_int * len(off))(*off)
            tok_a = (C.c_int * max(1, len(toks)))(*toks)
            cfg.procs = C.pointer(L.LogitsProcCfg(float(procs["repetition_penalty"]), int(procs["no_repeat_ngram_size"]),
                                                  int(procs["min_length"]), int(procs["min_new_tokens"]), len(words),
                                                  C.cast(off_a, C.POINTER(C.c_int)), C.cast(tok_a, C.POINTER(C.c_int))))
        cfg.want_logprobs = int(bool(want_logprobs))
        cfg.constraint = None  # (a Python attribute, not a field)
        if constraint is not None:
            trie, roots = constraint
            if roots.dtype != torch.int32 or not roots.is_contiguous() or roots.device != trie.child_off.device:
                raise ValueError("the constraint's roots must be a contiguous int32 tensor on the trie's device")
            cfg.constraint = L.ConstraintCfg(trie.child_off.data_ptr(), trie.child_tok.data_ptr(), trie.child_node.data_ptr(),
                                             trie.n_nodes, trie.n_edges, roots.data_ptr())
            cfg._constraint_keep = (trie.child_off, trie.child_tok, trie.child_node, roots)  # alive while the session runs
        return cfg

    def gen_workspace_bytes(self, cfg):
        """bytes of the session's workspace, with the buffers of the cfg's constraint when it carries one; 0 = settings this binding
        does not support"""
        self.gen_set_constraint(getattr(cfg, "constraint", None))
        try:
            return int(self._lib.klab_engine_gen_workspace_bytes(self._h, C.byref(cfg)))
        finally:
            self.gen_set_constraint(None)

    def gen_set_constraint(self, k):
        """arms the constraint (an _lib.ConstraintCfg, Engine.gen_cfg(constraint=) makes it) of the NEXT gen_begin, one-shot as the
        forced table; None disarms.  While one is armed gen_workspace_bytes answers for that session."""
        L.check(self._lib.klab_engine_gen_set_constraint(self._h, C.byref(k) if k is not None else None, L.stream_ptr()),
                "klab_engine_gen_set_constraint")

    def gen_set_forced(self, tokens, n_forced):
        """arms the forced-token table of the NEXT gen_begin (one-shot; gen_begin takes it whether it succeeds or not): tokens int64
        [B*n, ld] on the device, contiguous, row r's token of position p in tokens[r, p] for 1 <= p <= n_forced < ld.  A "force"
        session takes every position from it (scoring); a pick or sample session its first n_forced (a decoder prompt).  The
        engine keeps the tensor alive until the next gen_begin after that one."""
        if tokens.dtype != torch.int64 or tokens.dim() != 2 or not tokens.is_contiguous():
            raise ValueError("the forced-token table must be a contiguous int64 [rows, ld] tensor")
        L.check(self._lib.klab_engine_gen_set_forced(self._h, tokens.data_ptr(), tokens.shape[1], int(n_forced), L.stream_ptr()),
                "klab_engine_gen_set_forced")
        self._forced_armed = tokens

    def gen_attn_bytes(self, cfg):
        """bytes of the cross-attention maps a session with these settings can carry, f32 [n_dec_layers, B*n, max_length, Le]; 0 = none
        (beam search, or settings gen_workspace_bytes refuses)"""
        return int(self._lib.klab_engine_gen_attn_bytes(self._h, C.byref(cfg)))

    def gen_set_attn(self, buf):
        """arms the cross-attention maps of the NEXT gen_begin (one-shot; gen_begin takes the arming whether it succeeds or not): buf a
        contiguous f32 device tensor of at least gen_attn_bytes(cfg) bytes, read as [n_dec_layers, B*n, max_length, Le]; the session
        clears it and writes into [i, r, p] the head-mean cross-attention of layer i that produced row r's token of position p
        (column 0, columns not reached and everything after a row's EOS stay 0).  None disarms.  The engine keeps the tensor alive
        until the next gen_begin after that one."""
        if buf is None:
            L.check(self._lib.klab_engine_gen_set_attn(self._h, None, 0, L.stream_ptr()), "klab_engine_gen_set_attn")
            self._attn_armed = None
            return
        if buf.dtype != torch.float32 or not buf.is_contiguous() or not buf.is_cuda:
            raise ValueError("the cross-attention maps must be a contiguous float32 device tensor")
        L.check(self._lib.klab_engine_gen_set_attn(self._h, buf.data_ptr(), buf.numel() * 4, L.stream_ptr()), "klab_engine_gen_set_attn")
        self._attn_armed = buf

    def gen_begin(self, cfg, ws):
        """after an evaluation-mode forward (the prefill): the session's state, and position 1 from the prefill's position-0 logits"""
        self._forced, self._forced_armed = self._forced_armed, None  # (the session's table stays referenced)
        self._attn, self._attn_armed = self._attn_armed, None  # (... and its maps)
        self.gen_set_constraint(getattr(cfg, "constraint", None))  # (the cfg, kept in self._gen, keeps the tables referenced)
        L.check(self._lib.klab_engine_gen_begin(self._h, C.byref(cfg), ws.data_ptr(), L.stream_ptr()), "klab_engine_gen_begin")
        self._gen = cfg

    def gen_step(self, t, ws):
        """decoder over position t for all rows, then position t + 1"""
        L.check(self._lib.klab_engine_gen_step(self._h, int(t), ws.data_ptr(), L.stream_ptr()), "klab_engine_gen_step")

    def gen_going(self, ws, pos):
        """the one host sync per step: whether the session goes on after position pos (beam search: bits 1 (improvable) and 4 (live
        candidate), and 2 (open pool entry) with early_stopping True; sampling and pick: some row unfinished)"""
        p = self._lib.klab_engine_gen_stop_word(self._h, ws.data_ptr(), int(pos))
        if not p:
            raise ValueError("klab: bad argument to klab_engine_gen_stop_word")
        off = p - ws.data_ptr()
        w = int(ws[off:off + 4].view(torch.int32).item())
        if self._gen.mode != L.GEN_BEAM:
            return w != 0
        return bool((w & 1) and (w & 4) and (self._gen.early_stopping != 1 or (w & 2)))

    def gen_buffer(self, ws, name):
        """a view into ws -- "logits": [B*n, vocab], the logits gen_step decoded last; "tokens": [B*n] int64, the next step's inputs;
        "logprobs" (want_logprobs sessions): [B*n, max_length] f32, the log-probability of every token chosen so far; "nodes"
        (constrained sessions): [B*n, 1] int32, the trie node every row stood on when the last position was chosen"""
        rows, cols, dt = C.c_long(), C.c_long(), C.c_int()
        p = self._lib.klab_engine_gen_buffer(self._h, ws.data_ptr(), name.encode(), C.byref(rows), C.byref(cols), C.byref(dt))
        if not p:
            raise KeyError(name)
        tdt = torch.int64 if name == "tokens" else torch.int32 if name == "nodes" else torch.float32 if dt.value == L.F32 else torch.bfloat16
        off = p - ws.data_ptr()
        v = ws[off:off + rows.value * cols.value * tdt.itemsize].view(tdt)
        return v if name == "tokens" else v.view(rows.value, cols.value)

    def gen_result(self, ws, n, length):
        """beam search: (sequences [B*n, length = max_length] int64, scores [B*n] f32, generated lengths [B*n] int32) of the first n
        entries of the finished pools; sampling and pick: (the first `length` columns of the sequences [B*n, length] int64, None, None)"""
        B, n, length = self.shape[0], int(n), int(length)
        seq = torch.empty(B * n, length, dtype=torch.int64, device=ws.device)
        if self._gen.mode != L.GEN_BEAM:
            L.check(self._lib.klab_engine_gen_result(self._h, ws.data_ptr(), n, length, seq.data_ptr(), None, None, L.stream_ptr()),
                    "klab_engine_gen_result")
            return seq, None, None
        scores = torch.empty(B * n, dtype=torch.float32, device=ws.device)
        lens = torch.empty(B * n, dtype=torch.int32, device=ws.device)
        L.check(self._lib.klab_engine_gen_result(self._h, ws.data_ptr(), n, length, seq.data_ptr(), scores.data_ptr(), lens.data_ptr(),
                                                 L.stream_ptr()), "klab_engine_gen_result")
        return seq, scores, lens

    def gen_scores(self, ws, length, n_out=None, length_penalty=1.0, want_tokens=True):
        """a want_logprobs session's (token_logprobs [B*n, length] f32 or None, scores [B*n] f32 = sum / len ** length_penalty,
        lengths [B*n] int32 through the first EOS, order [B*n_out] int32: each image's n_out best rows by score, or None) -- one
        klab_gen_finalize launch, everything stays on the device"""
        rows, length = self.shape[0] * self._gen.n, int(length)
        dev = ws.device
        lp = torch.empty(rows, length, dtype=torch.float32, device=dev) if want_tokens else None
        scores = torch.empty(rows, dtype=torch.float32, device=dev)
        lens = torch.empty(rows, dtype=torch.int32, device=dev)
        order = torch.empty(self.shape[0] * int(n_out), dtype=torch.int32, device=dev) if n_out is not None else None
        L.check(self._lib.klab_engine_gen_scores(self._h, ws.data_ptr(), length, int(n_out or 0), float(length_penalty),
                                                 lp.data_ptr() if want_tokens else None, scores.data_ptr(), lens.data_ptr(),
                                                 order.data_ptr() if order is not None else None, L.stream_ptr()),
                "klab_engine_gen_scores")
        return lp, scores, lens, order

    def backward(self, segment, dloss=None):
        L.check(self._lib.klab_engine_backward(self._h, segment, dloss.data_ptr() if dloss is not None else None, L.stream_ptr()),
                "klab_engine_backward")

    def adam_step(self, m, v, lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, segment=None):
        """torch.optim.Adam's update for every parameter of the trainable T5 in one kernel (+ refreshed bf16 copies);
        segment = 0 / 1: only the tensors of that backward segment (both = one full step)."""
        if segment is not None:
            L.check(self._lib.klab_engine_adam_step_segment(self._h, int(segment), m.data_ptr(), v.data_ptr(), lr, beta1, beta2, eps,
                                                            weight_decay, bias_corr1, bias_corr2, L.stream_ptr()), "klab_engine_adam_step_segment")
            return
        L.check(self._lib.klab_engine_adam_step(self._h, m.data_ptr(), v.data_ptr(), lr, beta1, beta2, eps, weight_decay, bias_corr1,
                                                bias_corr2, L.stream_ptr()), "klab_engine_adam_step")

    def adam_layout(self):
        """(param data_ptrs in the table order of the fused Adam / AdamW steps, how many of them belong to backward segment 0)"""
        n = len(self.params["main"])
        buf, n0 = (C.c_long * n)(), C.c_int(0)
        rc = self._lib.klab_engine_adam_layout(self._h, n, buf, C.byref(n0))
        if rc <= 0:
            L.check(rc if rc < 0 else L.ERR_BADARG, "klab_engine_adam_layout")
        return [int(buf[i]) for i in range(rc)], int(n0.value)

    def adamw_step(self, m, v, group_of, groups, segment=None):
        """torch.optim.AdamW's update for every parameter of the trainable T5 in one kernel, whatever the number of parameter groups
        (+ refreshed bf16 copies).  group_of: int32 device tensor in adam_layout() order; groups: 1 .. 16 dicts of lr, beta1, beta2,
        eps, weight_decay, bias_corr1, bias_corr2 (host values, passed by value); segment = 0 / 1: only that backward segment."""
        L.check(self._lib.klab_engine_adamw_step(self._h, -1 if segment is None else int(segment), m.data_ptr(), v.data_ptr(),
                                                 group_of.data_ptr(), L.adamw_groups(groups), len(groups), L.stream_ptr()),
                "klab_engine_adamw_step")

    def ema_update(self, ema, w):
        """ema += w (p - ema) for every parameter of the trainable T5 in one kernel; ema: fp32 device tensor laid out like the "main"
        flat gradient buffer, w: host float in [0, 1] (passed by value).  The parameters are only read."""
        if ema.dtype != torch.float32 or not ema.is_contiguous() or ema.numel() < self.grad_elems["main"]:
            raise ValueError("the EMA buffer has to be a contiguous fp32 tensor of the flat gradient buffer's size")
        L.check(self._lib.klab_engine_ema_update(self._h, ema.data_ptr(), float(w), L.stream_ptr()), "klab_engine_ema_update")

    def ema_swap(self, ema):
        """exchange the bits of every parameter of the trainable T5 with its slice of `ema` in one kernel (+ refreshed bf16 copies of
        the parameters now in place); a second call restores both bit for bit."""
        if ema.dtype != torch.float32 or not ema.is_contiguous() or ema.numel() < self.grad_elems["main"]:
            raise ValueError("the EMA buffer has to be a contiguous fp32 tensor of the flat gradient buffer's size")
        L.check(self._lib.klab_engine_ema_swap(self._h, ema.data_ptr(), L.stream_ptr()), "klab_engine_ema_swap")

    def lora_layout(self):
        """{parameter name of the trainable T5: (arena element offset, flat-gradient element offset)}, -1 = none; fixed by the
        configuration (valid before and across bind)"""
        n = len(self.params["main"])
        buf = (C.c_long * (2 * n))()
        rc = self._lib.klab_engine_lora_layout(self._h, n, buf)
        if rc != n:
            L.check(rc if rc < 0 else L.ERR_BADARG, "klab_engine_lora_layout")
        return {spec.name: (int(buf[2 * i]), int(buf[2 * i + 1])) for i, spec in enumerate(self.params["main"])}

    def lora_set(self, desc):
        """registers the adapter table (ops.lora_table's int64 device tensor; the engine keeps it across re-binds and merges
        W + s B A into the arena behind every cast of the trainable weights), None clears it"""
        if desc is None:
            L.check(self._lib.klab_engine_lora_set(self._h, None, 0), "klab_engine_lora_set")
        else:
            assert desc.dtype == torch.int64 and desc.dim() == 2 and desc.shape[1] == 11 and desc.is_contiguous() and desc.is_cuda
            L.check(self._lib.klab_engine_lora_set(self._h, desc.data_ptr(), desc.shape[0]), "klab_engine_lora_set")
        self._lora_desc = desc  # (the engine reads the caller's tensor)

    def lora_grads(self, out, slab):
        """dA and dB of every registered adapter from the flat gradient buffer, in two launches on the current stream (after
        backward segments 0 and 1); out, slab: the fp32 device buffers ops.lora_table sized"""
        L.check(self._lib.klab_engine_lora_grads(self._h, out.data_ptr(), slab.data_ptr(), L.stream_ptr()), "klab_engine_lora_grads")

    def adafactor_sizes(self):
        """(state, scalar, scratch) element counts of the f32 buffers klab_engine_adafactor_step works on"""
        a, b, c = C.c_long(0), C.c_long(0), C.c_long(0)
        L.check(self._lib.klab_engine_adafactor_state_elems(self._h, C.byref(a), C.byref(b), C.byref(c)), "klab_engine_adafactor_state_elems")
        return a.value, b.value, c.value

    def adafactor_layout(self):
        """per tensor, in scalar-slot order: (param data_ptr, rows, cols, state_off, factored).  R = state[off : off + rows],
        C = state[off + round_up4(rows) : ... + cols]; an unfactored tensor's V = state[off : off + cols].  Synchronises."""
        n = self.adafactor_sizes()[1] // 4
        buf = (C.c_long * (10 * n))()
        rc = self._lib.klab_engine_adafactor_layout(self._h, n, buf)
        if rc != n:
            L.check(rc if rc < 0 else L.ERR_BADARG, "klab_engine_adafactor_layout")
        return [(buf[10 * i], buf[10 * i + 3], buf[10 * i + 4], buf[10 * i + 5], bool(buf[10 * i + 9])) for i in range(n)]

    def adafactor_step(self, state, m, scalars, scratch, beta2t, one_minus_beta2t, eps0, eps1, rel_step, clip_threshold, beta1,
                       one_minus_beta1, weight_decay, scale_parameter):
        """transformers' Adafactor update for every parameter of the trainable T5 in four launches (+ refreshed bf16 copies);
        m = None: no first moment"""
        L.check(self._lib.klab_engine_adafactor_step(self._h, state.data_ptr(), None if m is None else m.data_ptr(), scalars.data_ptr(),
                                                     scratch.data_ptr(), beta2t, one_minus_beta2t, eps0, eps1, rel_step, clip_threshold,
                                                     beta1, one_minus_beta1, weight_decay, int(bool(scale_parameter)), L.stream_ptr()),
                "klab_engine_adafactor_step")

    def set_bucket_events(self, on=True):
        """record the per-layer bucket events during backward (a data-parallel reducer is attached)"""
        L.check(self._lib.klab_engine_set_bucket_events(self._h, int(on)), "klab_engine_set_bucket_events")

    def bucket_wait(self, segment, i, stream):
        """`stream` (torch.cuda.Stream) waits until layer bucket i of the last backward of `segment` is final; False when the
        engine has no per-layer events for it (graph replay): the caller then waits for the whole segment."""
        rc = self._lib.klab_engine_bucket_wait(self._h, int(segment), int(i), stream.cuda_stream)
        if rc == L.ERR_UNSUPPORTED:
            return False
        L.check(rc, "klab_engine_bucket_wait")
        return True

    def get_rng(self):
        """(base seed, forwards since seeding) of the device-side dropout RNG; synchronises the current stream"""
        b, n = C.c_uint32(), C.c_uint32()
        L.check(self._lib.klab_engine_get_rng(self._h, C.byref(b), C.byref(n), L.stream_ptr()), "klab_engine_get_rng")
        return int(b.value), int(n.value)

    def set_rng(self, base, counter):
        L.check(self._lib.klab_engine_set_rng(self._h, int(base) & 0xFFFFFFFF, int(counter) & 0xFFFFFFFF, L.stream_ptr()), "klab_engine_set_rng")

    def set_graph(self, on=True):
        """replay the launch sequences as hipGraphs (inputs are staged, so any input tensors may be passed)."""
        L.check(self._lib.klab_engine_set_graph(self._h, int(on)), "klab_engine_set_graph")

    def probe_enable(self, on=True):
        L.check(self._lib.klab_engine_probe_enable(self._h, int(on)), "klab_engine_probe_enable")

    def probe_read(self, channel=0):
        """(launches, total_ms, total_flops) of a probe channel since probe_enable() -- 0: LM-head logits GEMM, 1: grouped
        weight-gradient launches; call after a synchronize."""
        n, ms, fl = C.c_int(), C.c_float(), C.c_double()
        L.check(self._lib.klab_engine_probe_read(self._h, int(channel), C.byref(n), C.byref(ms), C.byref(fl)), "klab_engine_probe_read")
        return n.value, ms.value, fl.value

    def buffer(self, name):
        rows, cols, dt = C.c_long(), C.c_long(), C.c_int()
        p = self._lib.klab_engine_buffer(self._h, name.encode(), C.byref(rows), C.byref(cols), C.byref(dt))
        if not p:
            raise KeyError(name)
        tdt = torch.float32 if dt.value == L.F32 else torch.bfloat16
        es = 4 if dt.value == L.F32 else 2
        off = p - self.workspace.data_ptr()
        return self.workspace[off:off + rows.value * cols.value * es].view(tdt).view(rows.value, cols.value)
