"""LoRA adapters for the native T5 (`MyModel.transformer`), in merged-weight form.

    from klab_multimodalmodel_amd import lora
    ad = lora.attach(model, r=8, alpha=16, targets=("q", "v"))      # freezes the base T5, returns a LoraAdapters
    opt = torch.optim.AdamW(ad.parameters(), lr=1e-3)               # ordinary small fp32 nn.Parameters
    loss = model(images, src, tgt); loss.backward(); opt.step(); opt.zero_grad()
    caps = model.generate(pixels, src_ids)                          # decodes with the adapters in place
    ad.save("style_a.pt"); ad.load("style_b.pt")                    # adapter weights only
    ad.merge_and_unload()                                           # W += s B A into the fp32 masters, base trainable again
    ad.detach()                                                     # or: drop the adapters, base as before attach

Semantics are PEFT's: for a target matrix W [out, in], lora_A [r, in] (kaiming-uniform with a = sqrt(5): U(-1/sqrt(in), 1/sqrt(in))),
lora_B [out, r] (zeros), s = alpha / r and W_eff = W + s lora_B @ lora_A.  The T5 weights here are not nn.Linear modules and the
projections run inside fused kernels, so there is no x A^T B^T side path: the engine's forward reads compute-dtype copies of the
weights from one arena, and `klab_lora_merge` writes W_eff into that arena right behind the cast of the masters (fp32 sum, one
rounding into the copy -- how a full fine-tune's master and copy relate); the backward leaves the full dW of every matrix in the
flat gradient buffer, and `klab_lora_grads` projects dA = s B^T dW and dB = s dW A^T out of it.  Everything between runs unchanged
on W_eff: fused attention, GEMMs, LM head, generate, score.

A merged form has no place for `lora_dropout` (PEFT applies it to the input of the A path only, which does not exist here): it is
not offered.  Also out of scope: per-module ranks, DoRA / rsLoRA, adapters on Swin or on the frozen language encoder, klab DDP
(reducing only the adapter gradients), and skipping the weight-gradient products of frozen tensors -- the step still computes every
dW, so LoRA here saves optimizer state, optimizer time and checkpoint size, not backward FLOPs.
"""
import math
from collections import OrderedDict

import torch
from torch import nn

TARGETS = ("q", "k", "v", "o", "wi", "wi_0", "wi_1", "wo")  # last component of the HF Linear names of a T5 block
R_MAX = 64


def linear_modules(param_names):
    """HF module names of the adaptable matrices among `param_names` (names of `model.transformer` parameters), in their order:
    `<module>.weight` whose module's last component is one of TARGETS -- never shared, lm_head, the norm weights or
    relative_attention_bias"""
    out = []
    for n in param_names:
        if n.endswith(".weight"):
            mod = n[:-len(".weight")]
            if mod.rsplit(".", 1)[-1] in TARGETS:
                out.append(mod)
    return out


def select_targets(param_names, targets):
    """(normalised targets tuple, HF module names they select among `param_names`).  targets: "all-linear" (every one of TARGETS that
    exists), one name or a sequence of names; applies to every block and every attention kind.  ValueError: an unknown name, or
    one that matches no tensor."""
    mods = linear_modules(param_names)
    present = [t for t in TARGETS if any(m.rsplit(".", 1)[-1] == t for m in mods)]
    if isinstance(targets, str):
        targets = tuple(present) if targets == "all-linear" else (targets,)
    targets = tuple(targets)
    if not targets:
        raise ValueError("LoRA: no target modules given")
    for t in targets:
        if t not in TARGETS:
            raise ValueError(f"LoRA: unknown target {t!r}: expected 'all-linear' or any of {TARGETS}")
        if t not in present:
            raise ValueError(f"LoRA: target {t!r} matches no tensor of this model (it has {tuple(present)})")
    targets = tuple(t for t in TARGETS if t in targets)  # canonical order, no duplicates
    return targets, [m for m in mods if m.rsplit(".", 1)[-1] in targets]


def init_adapter(out_features, in_features, r, generator=None):
    """(lora_A [r, in] ~ U(-1/sqrt(in), 1/sqrt(in)), lora_B [out, r] = 0) on the host: nn.init.kaiming_uniform_(a=sqrt(5)) of
    PEFT's LoraLayer; randomness from `generator` or torch's global CPU generator"""
    bound = 1.0 / math.sqrt(in_features)
    a = torch.empty(r, in_features, dtype=torch.float32).uniform_(-bound, bound, generator=generator)
    return a, torch.zeros(out_features, r, dtype=torch.float32)


def _check_hyper(r, alpha):
    if isinstance(r, bool) or not isinstance(r, int) or not 1 <= r <= R_MAX:
        raise ValueError(f"LoRA: `r` has to be an integer in [1, {R_MAX}], got {r!r}")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not math.isfinite(alpha) or alpha <= 0:
        raise ValueError(f"LoRA: `alpha` has to be a positive finite number, got {alpha!r}")


class LoraAdapters:
    """The adapters of one model: `parameters()` for the optimizer, `state_dict()` / `save` / `load` for the adapter weights
    alone, `merge_and_unload()` and `detach()` to end.  Built by `attach`."""

    def __init__(self, model, r, alpha, targets, modules, generator=None):
        self.model = model
        self.r, self.alpha, self.targets = int(r), float(alpha), tuple(targets)
        self.scale = self.alpha / self.r
        self.modules = list(modules)
        self._base = [model.transformer.get_parameter(m + ".weight") for m in self.modules]
        self._params = OrderedDict()
        for m, w in zip(self.modules, self._base):
            a, b = init_adapter(w.shape[0], w.shape[1], self.r, generator)
            self._params[m + ".lora_A.weight"] = nn.Parameter(a.to(w.device))
            self._params[m + ".lora_B.weight"] = nn.Parameter(b.to(w.device))
        self._flags = None     # requires_grad of every model.transformer parameter before attach
        self._table_key = None  # data pointers the device table was built from
        self._desc = self._plan = self._out = self._slab = None
        self._fp = None        # version fingerprint of base + adapters at the last loss forward of this binding
        self._live = False

    # ---- the parameters ----------------------------------------------------------------------------------------------------------
    def parameters(self):
        return list(self._params.values())

    def named_parameters(self):
        return list(self._params.items())

    def num_parameters(self):
        return sum(p.numel() for p in self._params.values())

    def state_dict(self):
        sd = OrderedDict((k, p.detach()) for k, p in self._params.items())
        sd["r"], sd["alpha"], sd["targets"] = self.r, self.alpha, tuple(self.targets)
        return sd

    def load_state_dict(self, sd):
        for key, mine in (("r", self.r), ("alpha", self.alpha), ("targets", tuple(self.targets))):
            if key not in sd:
                raise ValueError(f"LoRA state dict: {key!r} is missing")
            theirs = tuple(sd[key]) if key == "targets" else sd[key]
            if theirs != mine:
                raise ValueError(f"LoRA state dict: {key} = {theirs!r}, these adapters have {mine!r}")
        keys = [k for k in sd if k not in ("r", "alpha", "targets")]
        missing, extra = [k for k in self._params if k not in sd], [k for k in keys if k not in self._params]
        if missing or extra:
            raise ValueError(f"LoRA state dict: missing keys {missing[:3]}, unexpected keys {extra[:3]}")
        for k, p in self._params.items():
            if tuple(sd[k].shape) != tuple(p.shape):
                raise ValueError(f"LoRA state dict: size mismatch for {k}: {tuple(sd[k].shape)} vs {tuple(p.shape)}")
        with torch.no_grad():
            for k, p in self._params.items():
                p.copy_(sd[k].to(torch.float32))  # (bumps the version counter: the next forward merges again)

    def save(self, path):
        sd = self.state_dict()
        torch.save(OrderedDict((k, v.cpu() if torch.is_tensor(v) else v) for k, v in sd.items()), path)

    def load(self, path):
        self.load_state_dict(torch.load(path, map_location="cpu"))

    # ---- engine plumbing (called by MyModel) -----------------------------------------------------------------------------------
    def _check_live(self):
        if not self._live or self.model._lora is not self:
            raise RuntimeError("these LoRA adapters are no longer attached to their model")

    def _fingerprint(self):
        return sum(p._version for p in self.model.transformer.parameters()) + sum(p._version for p in self._params.values())

    def _note_forward(self):
        self._fp = self._fingerprint()

    def _current(self):
        """nothing wrote a base or an adapter parameter since the last loss forward of this binding"""
        if self._fp is None:
            return False
        if self._fingerprint() != self._fp:
            self._fp = None
            return False
        return True

    def _install(self):
        """(re)builds the device table when a tensor moved and registers it with the engine; the next forward casts and merges"""
        from . import ops
        self._fp = None
        dev = self._base[0].device
        if dev.type != "cuda":
            raise RuntimeError("klab LoRA runs on an MI355X (cuda/HIP device) only; there is no CPU fallback")
        for p in self._params.values():
            if p.device != dev:
                p.data = p.data.to(dev)  # the model was moved after attach: the adapters follow (the Parameters stay the same objects)
        key = tuple(t.data_ptr() for t in self._base) + tuple(p.data_ptr() for p in self._params.values())
        eng = self.model._engine
        if key != self._table_key:
            layout = eng.lora_layout()
            entries = []
            for m, w in zip(self.modules, self._base):
                aoff, goff = layout[m + ".weight"]
                if aoff < 0 or goff < 0:
                    raise NotImplementedError(f"LoRA: {m}.weight has no arena copy or no gradient slice in this engine")
                entries.append((w.data, self._params[m + ".lora_A.weight"].data, self._params[m + ".lora_B.weight"].data, aoff, goff,
                                self.scale))
            self._desc, self._plan, n_out, n_slab = ops.lora_table(entries)
            self._out = torch.empty(n_out, dtype=torch.float32, device=dev)
            self._slab = torch.empty(n_slab, dtype=torch.float32, device=dev)
            self._table_key = key
        if getattr(eng, "_lora_desc", None) is not self._desc:
            eng.lora_set(self._desc)

    def _grads(self, eng):
        """(dA, dB) of every adapter in `parameters()` order from the engine's flat dW: two launches on the current stream; views of one
        fresh buffer per backward (autograd may keep them as .grad)"""
        eng.lora_grads(self._out, self._slab)
        flat = self._out.clone()
        out = []
        for w, (n4, _rb, _so, db) in zip(self._base, self._plan):
            o, i = w.shape
            out.append(flat[4 * n4:4 * n4 + self.r * i].view(self.r, i))
            out.append(flat[db:db + o * self.r].view(o, self.r))
        return tuple(out)

    # ---- ending ----------------------------------------------------------------------------------------------------------------------
    def _remove(self):
        m = self.model
        if getattr(m._engine, "_lora_desc", None) is not None:
            m._engine.lora_set(None)
        for n, p in m.transformer.named_parameters():
            p.requires_grad_(self._flags.get(n, p.requires_grad))
        m._lora = None
        m._train_fp = None  # the arena may hold merged copies: the next forward casts the masters again
        self._live = False
        self._desc = self._plan = self._out = self._slab = self._table_key = None

    def detach(self):
        """drops the adapters: base weights and requires_grad flags as before attach; the next forward casts the plain masters"""
        self._check_live()
        self._remove()

    @torch.no_grad()
    def merge_and_unload(self):
        """W += s B A into the fp32 masters (one launch, the very fp32 values whose casts the arena holds: loss and generate are
        bit-identical before and after), then drops the adapters; the base is trainable again as before attach"""
        self._check_live()
        from . import ops
        m = self.model
        m._join_pending_update()
        self._install()
        ops.lora_merge(self._desc, to_master=True)
        self._remove()


def attach(model, r=8, alpha=16, targets=("q", "v"), generator=None):
    """Freezes `model.transformer` (the flags are recorded and come back with detach / merge_and_unload) and adds a rank-r adapter
    with s = alpha / r to every matrix `targets` names: any of q, k, v, o, wi, wi_0, wi_1, wo, or "all-linear", in every block and
    every attention kind (encoder self, decoder self, cross).  One r and one alpha per attach, 1 <= r <= 64.  lora_B starts at zero, so
    the model computes what it computed before until the first optimizer step.  There is no lora_dropout (see the module docstring).
    Returns the LoraAdapters; hand `ad.parameters()` to any torch optimizer."""
    if hasattr(model, "module") and hasattr(model, "reducer"):
        raise NotImplementedError("LoRA adapters on a klab-DDP-wrapped model are not implemented (only the adapter gradients would "
                                  "have to be reduced)")
    if getattr(model, "_reducer", None) is not None:
        raise NotImplementedError("this model is wrapped in klab DDP: LoRA adapters under DDP are not implemented (only the adapter "
                                  "gradients would have to be reduced)")
    if getattr(model, "_lora", None) is not None:
        raise RuntimeError("this model already has LoRA adapters: detach() or merge_and_unload() them first")
    if model.compute_dtype == "fp8":
        raise NotImplementedError("LoRA adapters with dtype='fp8' are not implemented: use bf16")
    _check_hyper(r, alpha)
    names = [n for n, _p in model.transformer.named_parameters()]
    targets, modules = select_targets(names, targets)
    for m in modules:
        w = model.transformer.get_parameter(m + ".weight")
        if w.dim() != 2 or w.shape[1] % 4:
            raise NotImplementedError(f"LoRA: {m}.weight {tuple(w.shape)} needs two dimensions and an input width that is a multiple of 4")
    ad = LoraAdapters(model, r, alpha, targets, modules, generator)
    model._join_pending_update()
    ad._flags = {n: p.requires_grad for n, p in model.transformer.named_parameters()}
    model.transformer.requires_grad_(False)
    model._lora = ad
    model._train_fp = None
    ad._live = True
    if ad._base[0].device.type == "cuda":  # else at the first bind
        try:
            ad._install()
        except Exception:
            ad._remove()
            raise
    return ad
