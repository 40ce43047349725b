"""Fused optimizers for the native MyModel: Adam, AdamW with per-group hyper-parameters (`FusedAdamW`,
`decay_param_groups`) and Adafactor (`FusedAdafactor`), a fused exponential moving average of the weights with an in-place swap
for evaluation (`WeightEMA`), and on-device gradient-norm clipping (`clip_grad_norm_`, `grad_norms`, at the end of the file).

Drop-in for the reference's `torch.optim.Adam(model.module.transformer.parameters(), lr=args.lr)` (ref/train.py:28): same
constructor arguments, same update rule (no amsgrad, L2 weight decay), `param_groups` / LR schedulers / `zero_grad` /
`state_dict` as usual.  When every parameter belongs to one klab MyModel whose gradients live in the engine's flat buffer
(the direct-gradient mode that `MyModel._direct_grads` / klab DDP use), `step()` is ONE kernel over all tensors that also
rewrites the bf16 copies the next forward's GEMMs read -- the engine's separate fp32->bf16 cast pass is skipped.  In every
other situation (foreign parameters, several param groups with different hyper-parameters, amsgrad, gradients that are not
views of the flat buffer) it silently delegates to `torch.optim.Adam`, so it is always safe to use.  Several groups stay on the
one-kernel path with `FusedAdamW`.

`step_in_backward=True` (opt-in; ONLY for loops in which every `backward()` is followed by `step()`, i.e. the reference's loop
with its default `--accumulation_steps 1`, ref/train.py:61-67, ref/modules/config.py:16): the update of backward segment 0
(LM head / shared embedding / decoder, ~70 % of the trainable parameters) is enqueued on a side stream as soon as that
segment's gradients are final (and, under klab DDP, averaged), so that the HBM-bound Adam kernel runs underneath the
latency-bound encoder backward; `step()` then updates segment 1 and joins.  Same arithmetic, same result; the first step and
every step after a change of circumstances (`_fast_ok`) run the ordinary way.  Measured on configs[1] (one MI355X): 6.67 ms/step
against 6.63 without -- the co-running streaming kernel slows the chain by as much as it hides -- so nothing turns it on by default.
"""
import contextlib
import math
import struct
import weakref

import torch
from torch.optim import Adam as _TorchAdam
from torch.optim import AdamW as _TorchAdamW
from torch.optim import Optimizer


# ---- which model owns these parameters, and do the fused paths apply to it ---------------------------------------------------------
def _owners(params):
    """(the klab MyModels that own some of `params`, whether every parameter has one): a model's trainable T5 carries `_klab_owner`"""
    owners, all_owned = [], True
    for p in params:
        ref = getattr(p, "_klab_owner", None)
        m = ref() if ref is not None else None
        if m is None:
            all_owned = False
        elif all(m is not o for o in owners):
            owners.append(m)
    return owners, all_owned


def _one_owner(params, allow_unowned=False):
    """the one klab MyModel that owns `params`, else None.  Parameters nobody owns are tolerated only on request (clipping: the
    kernels take any gradient; the optimizers and the average need the engine's table to list every tensor)."""
    owners, all_owned = _owners(params)
    return owners[0] if len(owners) == 1 and (all_owned or allow_unowned) else None


def _join_reductions(params):
    """gradients may still be in flight (klab DDP overlap_optimizer): join before torch reads them"""
    for m in _owners(params)[0]:
        m._join_pending_reduce()


def _trainable_t5_of(params, grads_in_flat):
    """(model, None) when `params` are exactly the trainable T5 of one bound klab MyModel -- with `grads_in_flat`, every `.grad`
    also a view of the engine's flat gradient buffer --, else (None, reason)."""
    model = _one_owner(params)
    if model is None:
        return None, "parameters not owned by one klab MyModel"
    if model._flat.get("main") is None or model._engine.shape is None:
        return None, "engine not bound yet"
    if not grads_in_flat:
        model._grad_targets()  # builds the parameter -> flat-buffer views if no backward has run yet
    views = {id(p): v for p, v, mn in (model._views or []) if mn == "main"}
    mine = {id(p) for p in params}
    if mine != {id(p) for p in model.transformer.ordered() if p.requires_grad} or set(views) != mine:
        return None, "not exactly the trainable T5 parameters"
    if grads_in_flat and any(p.grad is None or p.grad.data_ptr() != views[id(p)].data_ptr() for p in params):
        return None, "gradients are not views of the flat buffer"
    return model, None


class FusedAdam(Optimizer):
    _torch_cls = _TorchAdam  # the optimizer every other situation is delegated to

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, maximize=False,
                 step_in_backward=False):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize)
        super().__init__(params, defaults)
        self._steps = 0
        self._m = self._v = None
        self._owner = None
        self._fallback = None
        self._fb_reason = None
        self.step_in_backward = bool(step_in_backward)
        self._opt_stream = None
        self._bw_token = None  # forward token of the backward whose segment 0 was already updated
        self.in_backward_updates = 0  # how many segment-0 updates ran underneath a backward (tests, bench)

    def _hyper(self, steps):
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        return (float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]), 1.0 - b1 ** steps, 1.0 - b2 ** steps)

    def _launch(self, model, steps, segment=None):
        """the update number `steps` of every tensor, or of backward segment 0 / 1, on the current stream"""
        model._engine.adam_step(self._m, self._v, *self._hyper(steps), segment=segment)

    def _in_backward_ok(self, model):
        """may segment 0 be updated underneath this backward? (the groups' side of the question)"""
        return self._groups_ok() is None

    def _second_backward_error(self):
        return RuntimeError(f"{type(self).__name__}(step_in_backward=True) supports exactly one backward() per step(); with gradient "
                            f"accumulation construct it with step_in_backward=False")

    @torch.no_grad()
    def _segment_ready(self, model, seg):
        """called by the model's backward when segment `seg`'s gradients are final on the current stream (and their all-reduce,
        if any, is enqueued): update segment 0 underneath the rest of the backward"""
        if seg != 0 or self._fallback is not None or self._m is None:
            return
        if self._bw_token is not None:
            # a second backward() before step(): gradient accumulation (ref/train.py --accumulation_steps > 1).  The first
            # micro-batch's gradients were already applied to segment 0 underneath its backward -- the update is not what Adam
            # would have done with the accumulated sum.  The contract is one backward per step: say so instead of training wrong.
            # (_LossFn.backward raises the same error before it starts: this call is reached with fresh gradients only)
            raise self._second_backward_error()
        if self._owner is None or self._owner() is not model or not self._in_backward_ok(model):
            return
        flat = model._flat.get("main")
        if flat is None or self._m.shape != flat.shape or self._m.device != flat.device:
            return
        cur = torch.cuda.current_stream(flat.device)
        if self._opt_stream is None:
            self._opt_stream = torch.cuda.Stream(device=flat.device)
        self._opt_stream.wait_stream(cur)
        with torch.cuda.stream(self._opt_stream):
            red = getattr(model, "_reducer", None)
            if red is not None:
                red.finish_segment(0, flat.device)  # the current stream is the optimizer stream here
            self._launch(model, self._steps + 1, 0)
        self._bw_token = model._fwd_token
        self.in_backward_updates += 1
        model._pending_opt_stream = self._opt_stream

    def _all_params(self):
        return [p for g in self.param_groups for p in g["params"]]  # (torch refuses a parameter in two groups)

    def _find_owner(self):
        return _one_owner(self._all_params())

    def _groups_ok(self):
        """None when the groups' settings allow the one-kernel path, else the reason"""
        if len(self.param_groups) != 1:
            return "several param groups"
        g = self.param_groups[0]
        if g["amsgrad"] or g["maximize"]:
            return "amsgrad / maximize"
        return None

    def _fast_ok(self):
        """(model, None) when the one-kernel path applies, else (None, reason)."""
        why = self._groups_ok()
        if why is not None:
            return None, why
        return _trainable_t5_of(self._all_params(), grads_in_flat=True)

    def _moments(self, model):
        """(param, exp_avg view, exp_avg_sq view) of every trainable T5 tensor: the flat buffers are laid out like `model`'s flat
        gradient buffer"""
        for p, v, mn in model._views:
            if mn == "main" and p.requires_grad:
                off = v.storage_offset()
                yield p, self._m[off:off + p.numel()].view(p.shape), self._v[off:off + p.numel()].view(p.shape)

    # ---- torch.optim API --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        model, why = (None, "fallback already active") if self._fallback is not None else self._fast_ok()
        if model is None:
            if self._bw_token is not None:
                raise RuntimeError(f"{type(self).__name__}(step_in_backward=True): segment 0 was updated during backward() but step() cannot "
                                   f"take the fused path any more ({why})")
            _join_reductions(self._all_params())
            if self._fallback is None or self._fb_reason is None:  # (later steps keep the reason of the first)
                self._fb_reason = why
            self._step_fallback()
            return loss
        flat = model._flat["main"]
        if self._m is None or self._m.shape != flat.shape or self._m.device != flat.device:
            if self._bw_token is not None:
                raise RuntimeError(f"{type(self).__name__}(step_in_backward=True): the optimizer state changed between backward() and step()")
            self._m = torch.zeros_like(flat)
            self._v = torch.zeros_like(flat)
        self._steps += 1
        steps = self._steps
        seg0_done = self._bw_token is not None  # (reset by every step, set by every backward: one backward per step is the contract)
        self._bw_token = None
        if seg0_done:  # segment 0 was updated during the backward: the compute stream continues behind it
            torch.cuda.current_stream(flat.device).wait_stream(self._opt_stream)
            model._pending_opt_stream = None

        def launch():
            red = getattr(model, "_pending_reduce", None)
            if red is not None:  # klab DDP(overlap_optimizer=True): segment 0 is updated while segment 1 is still being reduced
                model._pending_reduce = None
                for seg in (0, 1):
                    if seg == 0 and seg0_done:
                        continue
                    red.finish_segment(seg)
                    self._launch(model, steps, seg)
                red.finish()  # any further segment (Swin) and the bookkeeping
            elif seg0_done:
                self._launch(model, steps, 1)
            else:
                self._launch(model, steps)

        launch()
        model._note_optimizer_step()
        self._owner = weakref.ref(model)
        model._optimizer_in_backward = weakref.ref(self) if self.step_in_backward else None
        return loss

    def _step_fallback(self):
        if self._fallback is None:
            self._fallback = self._torch_cls(self.param_groups, fused=all(p.is_cuda for g in self.param_groups for p in g["params"]) or None)
            self._fallback.param_groups = self.param_groups  # share the group dicts (LR schedulers act on ours)
            if self._m is not None:  # carry the fused state over (one-way)
                model = self._owner() if self._owner is not None else None
                if model is not None:
                    for p, m, v in self._moments(model):
                        self._fallback.state[p] = {
                            "step": torch.tensor(float(self._steps), device=p.device if self._fallback.defaults.get("fused") else "cpu"),
                            "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        self._fallback.step()

    def state_dict(self):
        """torch.optim.Adam-compatible: per-parameter `step`, `exp_avg`, `exp_avg_sq` (copies)."""
        if self._fallback is not None:
            return self._fallback.state_dict()
        model = self._owner() if self._owner is not None else None
        if model is not None and self._m is not None:
            for p, m, v in self._moments(model):
                self.state[p] = {"step": torch.tensor(float(self._steps)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """torch.optim.Adam-compatible.  The model must have been bound to a batch shape (one forward) so that the flat state
        layout is known; otherwise the loaded state is kept per parameter and the torch fallback continues from it."""
        super().load_state_dict(state_dict)
        model = self._find_owner()
        steps = 0
        if model is not None and model._flat.get("main") is not None:
            model._grad_targets()  # builds the parameter -> flat-buffer views if no backward has run yet
        why = self._loaded_state_refused()
        if why is not None:
            self._fb_reason = why
            model = None
        if model is not None and model._views:
            flat = model._flat["main"]
            self._m, self._v = torch.zeros_like(flat), torch.zeros_like(flat)
            for p, m, v in self._moments(model):
                st = self.state.get(p)
                if not st:
                    continue
                m.copy_(st["exp_avg"])
                v.copy_(st["exp_avg_sq"])
                steps = max(steps, int(float(st["step"])))
            self._owner = weakref.ref(model)
            self._steps = steps
            self._fallback = None
        else:  # no flat layout yet: continue with torch.optim.Adam on the loaded per-parameter state
            self._fallback = self._torch_cls(self.param_groups)
            self._fallback.param_groups = self.param_groups
            self._fallback.state = self.state

    def _loaded_state_refused(self):
        """why a state that load_state_dict has just put into self.state cannot live in the flat buffers, or None"""
        return None


class FusedAdamW(FusedAdam):
    """Drop-in for `torch.optim.AdamW` (decoupled weight decay, no amsgrad / maximize on the fused path): the same constructor, a
    parameter iterable or a list of group dicts, `param_groups` / LR schedulers / `zero_grad` / `state_dict` as usual -- the
    optimizer of the usual T5 fine-tuning recipe, with decay on the matrices and none on the norm weights and the position bias
    (`decay_param_groups`).

    When the union of the groups is exactly the trainable T5 of one bound klab MyModel (each parameter once), every `.grad` is a
    view of the engine's flat gradient buffer (FusedAdam's ownership test), there are at most 16 groups, none of them asks for
    amsgrad or maximize and all parameters share one step count, `step()` is ONE launch of csrc/adamw.hip whatever the number of
    groups (one per backward segment under `step_in_backward` / klab DDP `overlap_optimizer`, exactly as FusedAdam).  The groups'
    hyper-parameters are read from `param_groups` at every step and travel in the kernel's arguments, so a scheduler that moves
    each group's `lr` simply works and nothing is copied to or read from the device.  The kernel also rewrites the compute-dtype
    copies of the weights, so the next forward skips its cast.  Which group a tensor belongs to is a small device table in the
    engine's table order (`Engine.adam_layout()`), built once and again only when the model's gradient views are replaced or the
    groups' membership changes; a re-bind to another batch shape keeps it.

    One common step count: the flat state holds ONE `step` (the bias corrections are host scalars per group).  A loaded state whose
    parameters disagree about `step` continues in torch.  In every other situation too (CPU tensors, foreign parameters, amsgrad /
    maximize, more than 16 groups, an unbound engine) the step is `torch.optim.AdamW` on the shared group dicts, after any
    pending gradient reduction is joined and with the flat state carried over; `_fb_reason` says why."""
    _torch_cls = _TorchAdamW

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 step_in_backward=False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         step_in_backward=step_in_backward)
        self._gid = None        # int32 device tensor: the group of each tensor, in Engine.adam_layout() order
        self._gid_views = None  # the model's _views list and ...
        self._gid_key = None    # ... the groups' membership it was built for

    def _groups_ok(self):
        from . import _lib
        if not 1 <= len(self.param_groups) <= _lib.ADAMW_MAX_GROUPS:
            return f"more than {_lib.ADAMW_MAX_GROUPS} param groups"
        if any(g["amsgrad"] or g["maximize"] for g in self.param_groups):
            return "amsgrad / maximize"
        return None

    def _in_backward_ok(self, model):
        return self._groups_ok() is None and self._table_current(model)  # (the table is built at a step(), never inside a backward)

    def _membership(self):
        return tuple(tuple(id(p) for p in g["params"]) for g in self.param_groups)

    def _table_current(self, model):
        return self._gid is not None and self._gid_views is model._views and self._gid_key == self._membership()

    def _group_hyper(self, steps):
        out = []
        for g in self.param_groups:
            b1, b2 = g["betas"]
            out.append((float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]), 1.0 - b1 ** steps, 1.0 - b2 ** steps))
        return out

    def _group_table(self, model):
        """the device table of group ids for `model`'s engine"""
        if not self._table_current(model):
            ptrs, _n0 = model._engine.adam_layout()
            by_ptr = {p.data_ptr(): gi for gi, g in enumerate(self.param_groups) for p in g["params"]}
            if len(ptrs) != len(by_ptr) or any(q not in by_ptr for q in ptrs):
                raise RuntimeError("FusedAdamW: the engine's optimizer table does not list exactly this optimizer's parameters")
            host = torch.tensor([by_ptr[q] for q in ptrs], dtype=torch.int32).pin_memory()  # pinned: the upload does not synchronise
            self._gid = host.to(model._flat["main"].device, non_blocking=True)
            self._gid_views, self._gid_key = model._views, self._membership()
        return self._gid

    def _launch(self, model, steps, segment=None):
        model._engine.adamw_step(self._m, self._v, self._group_table(model), self._group_hyper(steps), segment=segment)

    def _loaded_state_refused(self):
        steps = {int(float(st["step"])) for st in self.state.values() if st and "step" in st}
        return "parameters with different step counts" if len(steps) > 1 else None


def decay_param_groups(tree_or_model, weight_decay, no_decay=("bias", "layer_norm")):
    """The usual two AdamW parameter groups over the trainable T5 of a klab MyModel (or over any module whose parameters carry
    HuggingFace state-dict names): `[{"params": [...], "weight_decay": weight_decay}, {"params": [...], "weight_decay": 0.0}]`.

    The rule is this project's: a parameter goes into the second group when its state-dict name contains one of the `no_decay`
    substrings.  For a T5 that is every `layer_norm.weight` / `final_layer_norm.weight` and `relative_attention_bias.weight` (T5
    has no bias vectors); everything else -- the embedding, the attention and feed-forward matrices, an untied LM head -- decays.
    Tied aliases (`encoder.embed_tokens.weight`, ...) are listed once, under the name that owns the tensor; parameters that do not
    require a gradient are left out."""
    tree = getattr(tree_or_model, "transformer", tree_or_model)
    decay, rest = [], []
    for name, p in tree.named_parameters():  # (named_parameters lists a shared tensor once)
        if not p.requires_grad:
            continue
        (rest if any(s in name for s in no_decay) else decay).append(p)
    return [{"params": decay, "weight_decay": float(weight_decay)}, {"params": rest, "weight_decay": 0.0}]


class FusedAdafactor(Optimizer):
    """Drop-in for `transformers.optimization.Adafactor` (the optimizer T5 v1.1 / Flan-T5 were pre-trained with): the same
    constructor, the same update rule, the same `state_dict()` keys (`step`, `RMS`, `exp_avg_sq_row` + `exp_avg_sq_col` or
    `exp_avg_sq`, `exp_avg` with `beta1`), so a state saved by either class loads into the other and continues.

    When the parameters are exactly the trainable T5 of one bound klab MyModel and their `.grad`s are views of the engine's flat
    gradient buffer (the test of `FusedAdam._fast_ok`), `step()` is four HIP launches over all tensors (csrc/adafactor.hip):
    statistics, their reduction, the update's norm, apply.  The step reads nothing back: `t`, `beta2t` and the relative step are
    host scalars, everything that depends on RMS(p) / RMS(u) stays on the device.  It has no floating-point atomics, so a step
    is bit-reproducible, and the apply pass also rewrites the compute-dtype copies the next forward's GEMMs read.  In every other
    situation (foreign parameters, CPU tensors, several groups, an unbound engine, a tensor shape the kernels do not cover) the
    same rule runs per parameter in plain torch, inside this file: `transformers` is never imported.  The state moves between
    the two forms as needed.

    Not supported: `step_in_backward` and segment-wise updates (FusedAdam's overlap with the backward / the DDP all-reduce).
    RMS(u) of a tensor needs all of its gradient, and the step joins a pending klab DDP reduction before it starts."""

    def __init__(self, params, lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0.0,
                 scale_parameter=True, relative_step=True, warmup_init=False):
        if lr is not None and relative_step:
            raise ValueError("Cannot combine manual `lr` and `relative_step=True` options")
        if warmup_init and not relative_step:
            raise ValueError("`warmup_init=True` requires `relative_step=True`")
        defaults = dict(lr=lr, eps=eps, clip_threshold=clip_threshold, decay_rate=decay_rate, beta1=beta1, weight_decay=weight_decay,
                        scale_parameter=scale_parameter, relative_step=relative_step, warmup_init=warmup_init)
        super().__init__(params, defaults)
        self._flat_live = False  # True: the state lives in the flat buffers below, self.state is stale
        self._steps = 0
        self._st = self._m = self._scal = self._scratch = None
        self._slots = None  # [(param, rows, cols, state_off, factored, m_off)] in scalar-slot order
        self._owner = None
        self._bound_key = None
        self._refused = None  # (model, binding) whose tensors the kernels turned down
        self._fb_reason = None

    # ---- the rule's host scalars ------------------------------------------------------------------------------------------
    @staticmethod
    def _rel_step(group, t):
        if group["relative_step"]:
            return min(1e-6 * t if group["warmup_init"] else 1e-2, 1.0 / math.sqrt(t))
        return group["lr"]

    _all_params = FusedAdam._all_params
    _find_owner = FusedAdam._find_owner

    def _fast_ok(self):
        """(model, None) when the fused path applies, else (None, reason): FusedAdam's ownership test."""
        if len(self.param_groups) != 1:
            return None, "several param groups"
        return _trainable_t5_of(self.param_groups[0]["params"], grads_in_flat=True)

    # ---- flat state <-> per-parameter (HF) state ------------------------------------------------------------------------------
    def _attach(self, model):
        """allocate the flat buffers for `model`'s bound engine; False when the kernels do not cover its tensors"""
        eng = model._engine
        try:
            n_state, n_scal, n_scratch = eng.adafactor_sizes()
            layout = eng.adafactor_layout()
        except NotImplementedError:
            return False
        by_ptr = {p.data_ptr(): (p, v.storage_offset()) for p, v, mn in model._views if mn == "main" and p.requires_grad}
        if len(layout) != len(by_ptr) or any(ptr not in by_ptr for ptr, *_ in layout):
            return False
        flat = model._flat["main"]
        self._slots = [(by_ptr[ptr][0], rows, cols, off, fact, by_ptr[ptr][1]) for ptr, rows, cols, off, fact in layout]
        self._st = torch.zeros(n_state, dtype=torch.float32, device=flat.device)
        self._scal = torch.zeros(n_scal, dtype=torch.float32, device=flat.device)
        self._scratch = torch.zeros(n_scratch, dtype=torch.float32, device=flat.device)
        self._m = torch.zeros_like(flat) if self.param_groups[0]["beta1"] is not None else None
        self._owner = weakref.ref(model)
        self._bound_key = model._bound_key
        return True

    def _slot_views(self, slot):
        p, rows, cols, off, fact, moff = slot
        if fact:
            c0 = off + ((rows + 3) & ~3)
            sq = {"exp_avg_sq_row": self._st[off:off + rows].view(p.shape[:-1]), "exp_avg_sq_col": self._st[c0:c0 + cols].view(p.shape[-1:])}
        else:
            sq = {"exp_avg_sq": self._st[off:off + cols].view(p.shape)}
        if self._m is not None:
            sq["exp_avg"] = self._m[moff:moff + p.numel()].view(p.shape)
        return sq

    def _export(self):
        """flat buffers -> self.state (copies, HF keys)"""
        if not self._flat_live:
            return
        for i, slot in enumerate(self._slots):
            st = {"step": self._steps, "RMS": self._scal[4 * i + 1].clone()}
            st.update({k: v.clone() for k, v in self._slot_views(slot).items()})
            self.state[slot[0]] = st

    def _import(self):
        """self.state -> flat buffers; the step count is the parameters' common one"""
        steps = 0
        self._st.zero_()
        if self._m is not None:
            self._m.zero_()
        dev = self._st.device
        rms = []  # one column write at the end instead of a device->host read per tensor
        for slot in self._slots:
            st = self.state.get(slot[0]) or {}
            for k, v in self._slot_views(slot).items():
                if k in st:
                    v.copy_(st[k])
            rms.append(torch.as_tensor(st.get("RMS", 0.0), dtype=torch.float32).to(dev).reshape(()))
            steps = max(steps, int(st.get("step", 0)))
        self._scal.view(-1, 4)[:, 1] = torch.stack(rms)
        self._steps = steps
        self.state.clear()
        self._flat_live = True

    # ---- torch.optim API ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        model, why = self._fast_ok()
        if model is not None and self._refused == (id(model), model._bound_key):
            model, why = None, "a tensor shape the Adafactor kernels do not cover"
        if model is not None and (self._st is None or self._owner is None or self._owner() is not model
                                  or (self._m is None) != (self.param_groups[0]["beta1"] is None)):
            self._export()
            self._flat_live = False
            if not self._attach(model):
                self._st = None
                self._refused = (id(model), model._bound_key)  # asked once per binding, not on every step
                model, why = None, "a tensor shape the Adafactor kernels do not cover"
        if model is None:
            _join_reductions(self._all_params())
            self._fb_reason = why
            self._export()
            self._flat_live = False
            self._step_fallback()
            return loss
        if not self._flat_live:
            self._import()
        if model._bound_key != self._bound_key:  # re-bound to another batch shape: same tensors, same layout
            if model._engine.adafactor_sizes() != (self._st.numel(), self._scal.numel(), self._scratch.numel()):
                raise RuntimeError("FusedAdafactor: the engine's Adafactor layout changed under a live optimizer state")
            self._bound_key = model._bound_key
        g = self.param_groups[0]
        self._steps += 1
        t = self._steps
        beta2t = 1.0 - math.pow(t, g["decay_rate"])
        model._join_pending_reduce()  # klab DDP(overlap_optimizer=True): RMS(u) needs every gradient, so the whole reduction is joined first
        model._join_pending_update(self._st.device)  # an in-backward update of another optimizer still writes the weights
        model._engine.adafactor_step(self._st, self._m, self._scal, self._scratch, beta2t, 1.0 - beta2t, float(g["eps"][0]), float(g["eps"][1]),
                                     float(self._rel_step(g, t)), float(g["clip_threshold"]), float(g["beta1"] or 0.0),
                                     1.0 - float(g["beta1"] or 0.0), float(g["weight_decay"]), g["scale_parameter"])
        model._note_optimizer_step()
        return loss

    def _step_fallback(self):
        """the same rule per parameter in plain torch, on self.state"""
        for group in self.param_groups:
            eps0, eps1 = group["eps"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Adafactor does not support sparse gradients.")
                grad = p.grad.float() if p.grad.dtype in (torch.float16, torch.bfloat16) else p.grad
                factored = grad.dim() >= 2
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["RMS"] = 0
                    if group["beta1"] is not None:
                        st["exp_avg"] = torch.zeros_like(grad)
                    if factored:
                        st["exp_avg_sq_row"] = grad.new_zeros(grad.shape[:-1])
                        st["exp_avg_sq_col"] = grad.new_zeros(grad.shape[:-2] + grad.shape[-1:])
                    else:
                        st["exp_avg_sq"] = torch.zeros_like(grad)
                else:
                    for k in ("exp_avg", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq"):
                        if k in st:
                            st[k] = st[k].to(grad)
                    if group["beta1"] is not None and "exp_avg" not in st:
                        st["exp_avg"] = torch.zeros_like(grad)
                w = p.float() if p.dtype in (torch.float16, torch.bfloat16) else p
                st["step"] = t = int(st["step"]) + 1
                st["RMS"] = rms_p = w.norm(2) / (w.numel() ** 0.5)
                lr = self._rel_step(group, t) * (max(eps1, rms_p) if group["scale_parameter"] else 1.0)
                beta2t = 1.0 - math.pow(t, group["decay_rate"])
                sq = grad ** 2 + eps0
                if factored:
                    row, col = st["exp_avg_sq_row"], st["exp_avg_sq_col"]
                    row.mul_(beta2t).add_(sq.mean(dim=-1), alpha=1.0 - beta2t)
                    col.mul_(beta2t).add_(sq.mean(dim=-2), alpha=1.0 - beta2t)
                    rf = (row / row.mean(dim=-1, keepdim=True)).rsqrt_().unsqueeze(-1)
                    u = torch.mul(rf, col.unsqueeze(-2).rsqrt()).mul_(grad)
                else:
                    v = st["exp_avg_sq"]
                    v.mul_(beta2t).add_(sq, alpha=1.0 - beta2t)
                    u = v.rsqrt().mul_(grad)
                rms_u = u.norm(2) / (u.numel() ** 0.5)
                u.div_((rms_u / group["clip_threshold"]).clamp_(min=1.0)).mul_(lr)
                if group["beta1"] is not None:
                    u = st["exp_avg"].mul_(group["beta1"]).add_(u, alpha=1 - group["beta1"])
                if group["weight_decay"] != 0:
                    w.add_(w, alpha=-group["weight_decay"] * lr)
                w.add_(-u)
                if w is not p:
                    p.copy_(w)

    def state_dict(self):
        """transformers.optimization.Adafactor-compatible (copies of the flat state when the fused path is live)."""
        self._export()
        sd = super().state_dict()
        if self._flat_live:
            self.state.clear()  # the flat buffers stay the live state; `sd` keeps the copies
        return sd

    def load_state_dict(self, state_dict):
        """transformers.optimization.Adafactor-compatible.  The loaded state is kept per parameter; the next `step()` moves it
        into the flat buffers when the fused path applies (the model must have been bound by one forward), else the torch rule
        continues from it."""
        super().load_state_dict(state_dict)
        self._flat_live = False
        self._steps = 0


# ---- exponential moving average of the weights (csrc/ema.hip) ---------------------------------------------------------------------
def _as_f32(x):
    """the double x rounded to the nearest f32, as a Python float: the scalar the kernel receives"""
    return struct.unpack("f", struct.pack("f", x))[0]


class WeightEMA:
    """Exponential moving average ("shadow") of the trainable weights, updated after every optimizer step; validation, `generate`,
    `score` and `save()` then run on the averaged weights inside `average_parameters()`:

        ema = WeightEMA(model, decay=0.999, warmup=True)
        ...
        opt.step(); ema.update()
        with ema.average_parameters():     # the averaged weights are the model's weights inside
            val_loss = model(...); caps = model.generate(...); model.save("ema.pth")

    `model` is a klab MyModel (its `.transformer` is tracked; a DDP wrapper is looked through), any `nn.Module`, or an iterable of
    parameters.  Parameters that do not require a gradient are left out, a tied tensor is tracked once.  The shadow is fp32 and
    starts as a copy of the parameters at construction.  The rule of `update()`:

        num_updates += 1
        decay_t = min(decay, (1 + num_updates) / (10 + num_updates))   with warmup, else decay
        w = float32(1.0 - decay_t)                                      formed in double
        shadow = shadow + w * (param - shadow)                          per element, in fp32

    `decay` has to lie in [0, 1).

    Fused path.  When the tracked parameters are exactly the trainable T5 of one bound klab MyModel (`FusedAdam`'s ownership test
    without its conditions on gradients: the average reads none), the shadow lives in ONE flat fp32 buffer shaped like the model's
    flat gradient buffer, `update()` is ONE launch whatever the number of tensors, and so is `swap()` -- and with it entering and
    leaving `average_parameters()`.  The swap exchanges the bits of parameters and shadow in place and rewrites the compute-dtype
    copies the forward's GEMMs read, so neither the first forward on the averaged weights nor the first one back on the raw
    weights pays the fp32 -> bf16 cast that `p.copy_()` would cause.  Both calls first order the current stream behind a pending
    in-backward optimizer update.

    In every other situation (the model is not bound yet, a foreign module, CPU tensors, parameters that are not exactly the
    trainable T5) the same rule runs per parameter in plain torch on per-parameter shadows; `_fb_reason` says why.  The state
    moves into the flat buffer at the first `update()` / `swap()` at which the fused path applies -- normally the first update,
    since the average is built before the first forward binds the engine -- and back when it stops applying.  A re-bind to
    another batch shape keeps the flat state (same tensors, same layout); a move of the model to another device moves the
    shadow with it.

    While the averaged weights are swapped in, the shadow holds the raw weights: `update()`, `state_dict()` and
    `load_state_dict()` raise RuntimeError.  `average_parameters()` swaps back when its body raises and is not re-entrant.
    Training inside the context is not supported.

    `state_dict()` is {"decay", "warmup", "num_updates", "shadow": {state-dict name: fp32 copy}}; for a module the names are those
    of its `state_dict()`, tied aliases included, so `model.transformer.load_state_dict(sd["shadow"])` works when every parameter
    is tracked.  `load_state_dict` is the inverse, before or after the model is bound and across the two forms.

    Data parallelism needs nothing: every rank holds the same weights and so computes the same average."""

    def __init__(self, model, decay=0.999, warmup=True):
        decay = float(decay)
        if not 0.0 <= decay < 1.0:  # (NaN fails too)
            raise ValueError(f"Invalid decay value: {decay}")
        self.decay, self.warmup, self.num_updates = decay, bool(warmup), 0
        if isinstance(model, torch.nn.Module):
            core = getattr(model, "module", model)
            tree = core.transformer if hasattr(core, "_engine") and hasattr(core, "transformer") else model
            named = list(tree.named_parameters())  # (lists a shared tensor once)
            every = list(tree.named_parameters(remove_duplicate=False))
        else:
            named, seen = [], set()
            for p in ([model] if isinstance(model, torch.Tensor) else model):
                if id(p) not in seen:
                    seen.add(id(p))
                    named.append((str(len(named)), p))
            every = named
        named = [(n, p) for n, p in named if p.requires_grad]
        if not named:
            raise ValueError("WeightEMA: no parameter requires a gradient")
        self._params = [p for _n, p in named]
        index = {id(p): i for i, p in enumerate(self._params)}
        self._names = [(n, index[id(p)]) for n, p in every if id(p) in index]  # every state-dict name of every tracked tensor
        with torch.no_grad():
            self._shadow = [p.detach().to(torch.float32, copy=True) for p in self._params]  # torch form; None while the flat buffer is live
        self._flat = None     # fused form: one fp32 buffer laid out like the owner's _flat["main"] ...
        self._offs = None     # ... and each tracked tensor's offset into it
        self._owner = None
        self._checked = None  # the binding (and gradient views) whose optimizer table was compared with the tracked tensors
        self._raw = None      # torch form, while swapped: the raw weights
        self._swapped = False
        self._fb_reason = None

    # ---- which form applies ---------------------------------------------------------------------------------------------------
    def _fast_ok(self):
        """(model, None) when the one-launch path applies, else (None, reason)"""
        model, why = _trainable_t5_of(self._params, grads_in_flat=False)
        if model is None:
            return None, why
        if model._bound_key is None:  # (moved with .to() since the last forward)
            return None, "engine not bound yet"
        flat = model._flat["main"]
        if any(p.device != flat.device or p.dtype != torch.float32 for p in self._params):
            return None, "parameters are not fp32 tensors on the engine's device"
        key = (model._bound_key, model._views)
        if self._checked is None or self._checked[0] != key[0] or self._checked[1] is not key[1]:
            try:
                ptrs, _n0 = model._engine.adam_layout()
            except NotImplementedError:
                return None, "the engine's optimizer table is unusable"
            if sorted(ptrs) != sorted(p.data_ptr() for p in self._params):
                return None, "the engine's optimizer table does not list exactly these tensors"
            self._checked = key
        return model, None

    def _slices(self):
        return [self._flat[off:off + p.numel()].view(p.shape) for p, off in zip(self._params, self._offs)]

    def _attach(self, model):
        """per-parameter shadows -> one flat buffer in the layout of the model's flat gradient buffer"""
        offs = {id(p): v.storage_offset() for p, v, mn in model._views if mn == "main"}
        self._flat = torch.zeros_like(model._flat["main"])
        self._offs = [offs[id(p)] for p in self._params]
        for dst, src in zip(self._slices(), self._shadow):
            dst.copy_(src)
        self._shadow = None
        self._owner = weakref.ref(model)

    def _detach(self):
        """flat buffer -> per-parameter shadows, on the parameters' devices"""
        self._shadow = [s.to(p.device, copy=True) for s, p in zip(self._slices(), self._params)]
        self._flat = self._offs = self._owner = None

    def _form(self):
        """the model of the fused path, or None for the torch path; the state moves to that form unless the averaged weights are
        swapped in (the way out of a swap is the way in)"""
        model, why = self._fast_ok()
        if self._swapped:
            return model if self._flat is not None else None
        if model is not None and self._flat is not None and (self._owner() is not model or self._flat.shape != model._flat["main"].shape
                                                            or self._flat.device != model._flat["main"].device):
            self._detach()
        if model is not None and self._flat is None:
            self._attach(model)
        elif model is None and self._flat is not None:
            self._detach()
        self._fb_reason = why
        return model

    def _not_swapped(self, what):
        if self._swapped:
            raise RuntimeError(f"WeightEMA.{what} while the averaged weights are swapped in (the shadow holds the raw weights): leave "
                               f"average_parameters() / call swap() first")

    # ---- the interface --------------------------------------------------------------------------------------------------------
    def decay_at(self, num_updates):
        """decay_t of update number `num_updates` (1-based)"""
        return min(self.decay, (1.0 + num_updates) / (10.0 + num_updates)) if self.warmup else self.decay

    @torch.no_grad()
    def update(self):
        """one step of the rule above; call it after every optimizer step"""
        self._not_swapped("update()")
        model = self._form()
        self.num_updates += 1
        w = _as_f32(1.0 - self.decay_at(self.num_updates))
        if model is not None:
            model._join_pending_update()
            with torch.cuda.device(self._flat.device):
                model._engine.ema_update(self._flat, w)
            return
        for i, p in enumerate(self._params):
            s = self._shadow[i]
            if s.device != p.device:
                s = self._shadow[i] = s.to(p.device)
            s.add_(p.detach().to(torch.float32) - s, alpha=w)

    @torch.no_grad()
    def swap(self):
        """exchange parameters and shadow: the first call puts the averaged weights into the model, the second the raw ones back,
        bit for bit"""
        model = self._form()
        if self._flat is not None and model is not None:
            model._join_pending_update()
            with torch.cuda.device(self._flat.device):
                model._engine.ema_swap(self._flat)
            model._note_optimizer_step()  # the compute-dtype copies are those of the weights now in place
        elif self._flat is not None:  # swapped in by the kernel, and the fused path is gone: the same exchange tensor by tensor
            for p, s in zip(self._params, self._slices()):
                tmp = p.detach().to(s.device, copy=True)
                p.copy_(s)
                s.copy_(tmp)
        elif not self._swapped:
            self._raw = [p.detach().clone() for p in self._params]
            for p, s in zip(self._params, self._shadow):
                p.copy_(s)
        else:
            for p, r in zip(self._params, self._raw):
                p.copy_(r)
            self._raw = None
        self._swapped = not self._swapped

    @contextlib.contextmanager
    def average_parameters(self):
        """context in which the averaged weights are the model's weights; the raw ones come back bit for bit, on exceptions too"""
        if self._swapped:
            raise RuntimeError("WeightEMA.average_parameters() is not re-entrant: the averaged weights are already swapped in")
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    @torch.no_grad()
    def state_dict(self):
        self._not_swapped("state_dict()")
        self._form()
        vals = self._slices() if self._flat is not None else self._shadow
        copies = [v.detach().clone() for v in vals]
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates,
                "shadow": {name: copies[i] for name, i in self._names}}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        self._not_swapped("load_state_dict()")
        shadow = state_dict["shadow"]
        first = {}
        for name, i in self._names:
            if name in shadow:
                first.setdefault(i, name)
        missing = [name for name, i in self._names if i not in first]
        if missing:
            raise KeyError(f"WeightEMA.load_state_dict: missing shadow key(s) {missing[:5]}{'...' if len(missing) > 5 else ''}")
        self._form()
        vals = self._slices() if self._flat is not None else self._shadow
        for i, v in enumerate(vals):
            src = shadow[first[i]]
            if tuple(src.shape) != tuple(v.shape):
                raise RuntimeError(f"size mismatch for {first[i]}: saved {tuple(src.shape)} vs tracked {tuple(v.shape)}")
            v.copy_(src)
        decay = float(state_dict["decay"])
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"Invalid decay value: {decay}")
        self.decay, self.warmup, self.num_updates = decay, bool(state_dict["warmup"]), int(state_dict["num_updates"])


# ---- gradient-norm clipping (csrc/grad_clip.hip) ------------------------------------------------------------------------------------
_CLIP_CACHE = {}  # (device, ((data_ptr, numel), ...)) -> _ClipState, for gradients no klab model owns
_CLIP_CACHE_MAX = 8


class _ClipState:
    """the device table of one set of gradient tensors, its fp64 partials and the result words: norms[0 .. nt - 1], the total at
    [nt], the clip coefficient at [nt + 1]"""

    def __init__(self, grads):
        from . import ops
        self.nt = len(grads)
        self.desc, self.nparts = ops.grad_table(grads)
        dev = grads[0].device
        self.parts = torch.empty(self.nparts, dtype=torch.float64, device=dev)
        self.res = torch.zeros(self.nt + 2, dtype=torch.float32, device=dev)


def _clip_native(params, grads, norm_type):
    """(state, owner) when the kernels apply to `grads` (the gradients of `params` that are not None), else (None, why)"""
    if norm_type != 2.0 and norm_type != math.inf:
        return None, "norm_type is neither 2 nor inf"
    dev = grads[0].device
    if dev.type != "cuda":
        return None, "gradients are not on a GPU"
    key = []
    for g in grads:
        if g.dtype != torch.float32 or g.device != dev or g.layout != torch.strided or not g.is_contiguous() or g.numel() == 0:
            return None, "a gradient is not a contiguous fp32 tensor on the one device"
        key.append((g.data_ptr(), g.numel()))
    key = tuple(key)
    if len({k[0] for k in key}) != len(key):
        return None, "a gradient tensor is listed twice"
    from . import _lib
    try:
        _lib.load()
    except (_lib.KlabError, OSError, AttributeError):
        return None, "the library does not load"
    owner = _one_owner(params, allow_unowned=True)
    if owner is not None:
        # kept on the model until it is re-bound: `_views` is a new list after every rebind (`_apply`, `_engine_for`)
        owner._grad_targets()
        cache = getattr(owner, "_clip_cache", None)
        if cache is None or cache[0] is not owner._views:
            cache = owner._clip_cache = (owner._views, {})
        states = cache[1]
    else:
        states = _CLIP_CACHE
    st = states.get((dev, key))
    if st is None:
        if len(states) >= _CLIP_CACHE_MAX:
            states.clear()
        with torch.cuda.device(dev):
            st = states[(dev, key)] = _ClipState(grads)
    return st, owner


def _clip_join(owner, dev):
    """order the current stream behind everything that still writes `owner`'s gradients or weights"""
    opt = owner._optimizer_in_backward() if owner._optimizer_in_backward is not None else None
    if opt is not None and opt._bw_token is not None:
        raise RuntimeError("clip_grad_norm_ needs the whole gradient before any update, but FusedAdam(step_in_backward=True) has "
                           "already updated segment 0 underneath this backward(); construct the optimizer with step_in_backward=False")
    owner._join_pending_reduce()  # klab DDP(overlap_optimizer=True): the last all-reduces are not joined yet
    owner._join_pending_update(dev)


def _clip_norms(st, owner, norm_type):
    from . import ops
    dev = st.res.device
    if owner is not None:
        _clip_join(owner, dev)
    with torch.cuda.device(dev):
        ops.grad_norm(st.desc, st.parts, st.res, kind=0 if norm_type == 2.0 else 1, nparts=st.nparts)


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """`torch.nn.utils.clip_grad_norm_` with the same signature, return value and messages.  For contiguous fp32 gradients on one
    GPU and `norm_type` 2 or inf it is three launches whatever the number of tensors (csrc/grad_clip.hip): the norm in one read of
    the gradients, and a scale pass that stores nothing unless the gradients are really clipped.  No host read (unless
    `error_if_nonfinite`), the gradients stay where they are (FusedAdam / FusedAdafactor keep their fused paths).  The total is
    accumulated in fp64: finite where torch's fp32 squares overflow, and the same bits on every run.  In every other case
    torch's function is called with the same arguments."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    else:
        parameters = list(parameters)  # (may be a generator, and torch's function would need it again)
    grads = [p.grad for p in parameters if p.grad is not None]
    max_norm, norm_type = float(max_norm), float(norm_type)
    if len(grads) == 0:
        return torch.tensor(0.0)
    st, owner = _clip_native(parameters, grads, norm_type)
    if st is None:
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type, error_if_nonfinite, foreach)
    from . import ops
    _clip_norms(st, owner, norm_type)
    total = st.res[st.nt]
    if error_if_nonfinite and not bool(torch.isfinite(total)):
        raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be "
                           "clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                           "`error_if_nonfinite=False`")
    with torch.cuda.device(st.res.device):
        ops.grad_clip(st.desc, st.res[st.nt:st.nt + 1], max_norm, st.res[st.nt + 1:st.nt + 2])
    return total.clone()  # the result words are written again by the next call


@torch.no_grad()
def grad_norms(parameters_or_model, norm_type=2.0):
    """(names, norms): the norm of every gradient and, last, of all of them, as the fp32 device tensor [nt + 1] that ONE
    klab_grad_norm call writes -- the per-parameter curve of a training log at the cost of the clipping's own norm pass, with no
    host read.  `names` are the HF state-dict names (`transformer.…`, `image_model.…`) for a klab MyModel, else the indices into
    the given parameters.  Parameters without a gradient are left out.  NotImplementedError where the kernels do not apply
    (see clip_grad_norm_)."""
    if isinstance(parameters_or_model, torch.nn.Module):
        named = [(n, p) for n, p in parameters_or_model.named_parameters() if p.requires_grad]
    elif isinstance(parameters_or_model, torch.Tensor):
        named = [(0, parameters_or_model)]
    else:
        named = list(enumerate(parameters_or_model))
    named = [(n, p) for n, p in named if p.grad is not None]
    names, params = [n for n, _p in named], [p for _n, p in named]
    norm_type = float(norm_type)
    if not params:
        raise NotImplementedError("grad_norms: no parameter has a gradient")
    st, owner = _clip_native(params, [p.grad for p in params], norm_type)
    if st is None:
        raise NotImplementedError(f"grad_norms needs the native path: {owner}")
    _clip_norms(st, owner, norm_type)
    return names, st.res[:st.nt + 1].clone()
