"""Drop-in mirror of the reference's `models/model.py::MyModel` (ref/models/model.py:8-42).

Same constructor (`MyModel(args)`), same `forward(images, source_encoding, target_encoding=None,
return_loss=True)`, same `save` / `load`, same attributes (`.transformer`, `.image_model`,
`.language_model`) and the same state-dict key schema as the HuggingFace modules the reference
wraps -- but forward + backward run in the native engine (libklab_mm.so), not in `transformers`.
`train.py` (ref/train.py) works unchanged: `.to(device)`, `DDP(model)`, `Adam(model.module.
transformer.parameters())`, `model.module.transformer.train()/eval()`, `loss.item()`,
`loss.backward()`, `model.module.save(...)`.
"""
import math
import os
from typing import Dict, List

import torch
from torch import nn

from .. import hf_io
from ..engine import Engine, SwinConfig, T5Config
from ..logits_proc import logits_processor_settings

TIED_T5 = ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight", "lm_head.weight")  # HF/t5:902-906


def tied_t5(cfg: T5Config):
    """aliases of `shared.weight` in a T5ForConditionalGeneration state dict: the LM head only when the config ties it (T5 v1.1 /
    Flan-T5 keep `lm_head.weight` as a parameter of its own)"""
    return TIED_T5 if cfg.tie_word_embeddings else TIED_T5[:2]


class _Node(nn.Module):
    """anonymous container so that dotted HuggingFace names become real module paths."""


class HFTree(nn.Module):
    """Parameters registered under HuggingFace state-dict names."""

    def __init__(self, specs, tied: Dict[str, str] = None):
        super().__init__()
        self._order: List[str] = []
        self._tied = tuple((tied or {}).keys())
        for spec in specs:
            self._register(spec.name, nn.Parameter(torch.empty(spec.shape, dtype=torch.float32)))
            self._order.append(spec.name)
        for alias, target in (tied or {}).items():
            self._register(alias, self.get_parameter(target))

    def _register(self, dotted, param):
        parts = dotted.split(".")
        mod = self
        for p in parts[:-1]:
            if not hasattr(mod, p):
                mod.add_module(p, _Node())
            mod = getattr(mod, p)
        mod.register_parameter(parts[-1], param)

    def ordered(self):
        return [self.get_parameter(n) for n in self._order]


def _init_t5_(tree: HFTree, cfg: T5Config, gen):
    """statistics of HF `_init_weights` (HF/t5:562-616), initializer_factor 1."""
    d, dk, h, ff = cfg.d_model, cfg.d_kv, cfg.num_heads, cfg.d_ff
    with torch.no_grad():
        for n, p in tree.named_parameters():
            if n in tree._tied:
                continue
            if n.endswith("layer_norm.weight"):
                p.fill_(1.0)
                continue
            std = 1.0
            if n.endswith(".q.weight"):
                std = (d * dk) ** -0.5
            elif n.endswith(".k.weight") or n.endswith(".v.weight"):
                std = d ** -0.5
            elif n.endswith(".o.weight"):
                std = (h * dk) ** -0.5
            elif n.endswith(("wi.weight", "wi_0.weight", "wi_1.weight")):
                std = d ** -0.5
            elif n.endswith("wo.weight"):
                std = ff ** -0.5
            elif n.endswith("relative_attention_bias.weight"):
                std = d ** -0.5
            p.copy_(torch.randn(p.shape, generator=gen) * std)


def _init_swin_(tree: HFTree, cfg: SwinConfig, gen):
    """statistics of HF `_init_weights` (HF/swinv2:873-886): N(0, 0.02) weights, zero biases, unit LayerNorm, log(10) scale."""
    with torch.no_grad():
        for n, p in tree.named_parameters():
            if n.endswith("logit_scale"):
                p.fill_(float(torch.log(torch.tensor(10.0))))
            elif "norm" in n.split(".")[-2] or n.startswith("layernorm"):
                p.fill_(1.0 if n.endswith("weight") else 0.0)
            elif n.endswith("bias"):
                p.zero_()
            else:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.02)


class _LossFn(torch.autograd.Function):
    """autograd boundary: one node for the whole forward; backward runs the engine's segments."""

    @staticmethod
    def forward(ctx, model, want_grad, pixels, src, tgt, *params):
        eng = model._engine_for(pixels, src, tgt)
        weights, model._loss_weights_next = model._loss_weights_next, None
        teacher, model._teacher_next = model._teacher_next, None
        eps, z = model._loss_options["label_smoothing"], model._loss_options["z_loss"]
        alpha, temp = model._distill_options["distill_alpha"], model._distill_options["distill_temperature"]
        if teacher is not None:  # (the binding exists only now; nothing is armed yet)
            model._check_teacher_alias(eng, teacher)
        # a fresh tensor per step, written by the cross-entropy kernel itself (no copy launch behind it)
        out = torch.empty(1, device=pixels.device, dtype=torch.float32)
        direct_loss = eng.set_loss_out(out)
        model._logits_valid = False
        # the engine keeps a device-side counter RNG: the base only (re)seeds it, every forward advances it
        try:
            eng.set_loss_options(eps, z, weights)
            eng.set_weight_norm(model._weight_norm == "count")
            eng.set_distill(alpha, temp, teacher)
            eng.forward(pixels, src, tgt, training=int(model.transformer.training) | (2 if model._frozen_unchanged() else 0) | (4 if model._trainable_current() else 0),
                        seed=model._seed_base, want_grad=want_grad)
        except Exception:
            eng.set_loss_out(None)  # a forward that failed before its cross-entropy must not leave the one-shot pointer armed
            eng.set_loss_options(eps, z, None)  # ... nor the one-shot loss weights
            eng.set_distill(alpha, temp, None)  # ... nor the one-shot teacher
            raise
        model._token_losses_valid = True
        model._token_kl_valid = teacher is not None
        model._logits_valid = not want_grad  # (with gradients the loss kernel has replaced the logits by d loss / d logits)
        model._token_losses_shape = tuple(tgt.shape)
        ctx.model = model
        ctx.eng = eng
        ctx.nparams = len(params)
        # LoRA (lora.attach): the adapter parameters travel behind the base parameters; the arena now holds W + s B A of these versions
        ctx.nlora = len(model._lora.parameters()) if model._lora is not None else 0
        if model._lora is not None:
            model._lora._note_forward()
        model._fwd_token += 1
        ctx.token = model._fwd_token
        return out[0] if direct_loss else eng.loss_view[0].clone()

    @staticmethod
    def backward(ctx, gout):
        model, eng = ctx.model, ctx.eng
        if ctx.token != model._fwd_token or eng is not model._engine:
            raise RuntimeError("klab MyModel: backward() must follow its own forward() (activations live in one workspace)")
        opt = model._optimizer_in_backward() if model._optimizer_in_backward is not None else None
        if opt is not None and opt._bw_token is not None:
            # a second backward() before step() (gradient accumulation): segment 0 was already updated underneath the first one.
            # The gradients are no longer "fresh" now, so _segment_ready below would never be asked: say it here.
            raise opt._second_backward_error()
        if ctx.nlora and model._lora is None:
            raise RuntimeError("klab MyModel: the LoRA adapters of this forward() were removed before its backward()")
        g = gout.detach().to(torch.float32).contiguous().view(1)
        direct = model._direct_grads
        targets = model._grad_targets()
        nseg = 3 if model.args.image_model_train else 2
        if not direct:
            for seg in range(nseg):
                eng.backward(seg, g)
                if model._segment_hook is not None:
                    model._segment_hook(seg)
        else:
            # .grad tensors alias the flat buffers the engine is about to overwrite.  Per flat buffer: parameters whose
            # .grad is None get fresh gradients; parameters that still hold a gradient (accumulation steps, or the Swin
            # gradients the reference never zeroes) keep the running sum.
            state, held = {}, {}
            for mname in ("main", "swin"):
                ps = [p for p, _v, mn in model._views if mn == mname and p.requires_grad]
                if model._flat.get(mname) is None or not ps:
                    continue
                n_set = sum(p.grad is not None for p in ps)
                state[mname] = "fresh" if n_set == 0 else ("all" if n_set == len(ps) else "mixed")
                if n_set:
                    held[mname] = model._flat[mname].clone()
            seg_model = ("main", "main", "swin")

            def settle(mname):
                st = state.get(mname)
                if st == "all":
                    model._flat[mname].add_(held[mname])  # every .grad aliases the flat buffer: one fused add
                elif st is not None:
                    for p, view, mn in model._views:
                        if mn != mname or not p.requires_grad:
                            continue
                        if p.grad is None:
                            p.grad = view
                        elif st == "mixed":
                            off = view.storage_offset()
                            view.add_(held[mname][off:off + view.numel()].view(view.shape))

            for seg in range(nseg):
                eng.backward(seg, g)
                last_of_model = seg == nseg - 1 or seg_model[seg + 1] != seg_model[seg]
                if state.get(seg_model[seg]) == "fresh":
                    if model._segment_hook is not None:
                        model._segment_hook(seg)
                    opt = model._optimizer_in_backward() if model._optimizer_in_backward is not None else None
                    if opt is not None and seg_model[seg] == "main":
                        opt._segment_ready(model, seg)  # optim.FusedAdam(step_in_backward=True)
                    if last_of_model:
                        settle(seg_model[seg])
                elif last_of_model:
                    settle(seg_model[seg])
                    if model._segment_hook is not None:
                        for s2 in range(nseg):
                            if seg_model[s2] == seg_model[seg]:
                                # the running sums were added on the current stream AFTER the engine's per-layer events:
                                # the reducer must order itself behind the stream, not behind those events
                                model._segment_hook(s2, False)
            # dA and dB are projected out of the full dW the segments left in the flat buffer, on this stream behind them
            return (None,) * (5 + ctx.nparams - ctx.nlora) + (model._lora._grads(eng) if ctx.nlora else ())
        grads = []
        views = {id(p): v for p, v in targets}
        for p in model._trainable():
            grads.append(views[id(p)])
        return (None, None, None, None, None) + tuple(grads) + (model._lora._grads(eng) if ctx.nlora else ())


class MyModel(nn.Module):
    def __init__(self, args, _configs=None, _state_dicts=None, _seed=0, dtype=None):
        super().__init__()
        self.args = args
        self.result_dir = args.result_dir
        if _configs is None:
            lang_cfg, lang_sd = hf_io.resolve(args.language_model_name, "t5")          # ref/models/model.py:14
            swin_cfg, swin_sd = hf_io.resolve(args.image_model_name, "swin")           # :15
            main_cfg, main_sd = hf_io.resolve(args.transformer_model_name, "t5")       # :17
        else:
            swin_cfg, lang_cfg, main_cfg = _configs
            swin_sd, lang_sd, main_sd = _state_dicts or (None, None, None)
        self.swin_cfg, self.lang_cfg, self.main_cfg = swin_cfg, lang_cfg, main_cfg
        dt = dtype or os.environ.get("KLAB_DTYPE", "bf16")
        # "fp8" (BASELINE configs[4]): bf16 storage and backward, forward Linear GEMMs on fp8 MFMA with per-row scales
        self.compute_dtype = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp8": "fp8", torch.bfloat16: torch.bfloat16,
                              torch.float32: torch.float32}[dt]
        self._engine = Engine(swin_cfg, lang_cfg, main_cfg, self.compute_dtype, bool(args.image_model_train))
        tied = {a: "shared.weight" for a in tied_t5(main_cfg)}
        self.language_model = HFTree(self._engine.params["lang"], {"encoder.embed_tokens.weight": "shared.weight"})
        self.image_model = HFTree(self._engine.params["swin"])
        self.transformer = HFTree(self._engine.params["main"], tied)
        gen = torch.Generator().manual_seed(_seed)
        for tree, cfg, sd, init in ((self.image_model, swin_cfg, swin_sd, _init_swin_), (self.language_model, lang_cfg, lang_sd, _init_t5_),
                                    (self.transformer, main_cfg, main_sd, _init_t5_)):
            if sd is None:
                init(tree, cfg, gen)
            else:
                self._load_tree(tree, sd)
        self.language_model.requires_grad_(False)                    # ref/models/model.py:14
        self.image_model.requires_grad_(bool(args.image_model_train))  # :15
        # from_pretrained returns eval-mode modules and the reference only ever toggles .transformer
        self.language_model.eval()
        self.image_model.eval()
        self.transformer.eval()
        self._bound_key = None
        self._flat = {}
        self._views = None
        self._direct_grads = False
        self._segment_hook = None
        self._optimizer_in_backward = None  # weakref to an optim.FusedAdam(step_in_backward=True) after its first fused step
        self._pending_opt_stream = None  # stream of an in-backward optimizer update that step() has not joined yet
        self._reducer = None  # klab DDP's SegmentReducer
        self._lora = None  # lora.LoraAdapters while adapters are attached (lora.attach)
        self._pending_reduce = None  # klab DDP(overlap_optimizer=True): reducer whose last all-reduces are not joined yet
        self.use_graph = os.environ.get("KLAB_GRAPH", "0") == "1"  # hipGraph replay of the engine's launch sequences
        self._seed_base = torch.initial_seed() & 0xFFFFFFFF
        self._pending_rng = None  # (base, counter) restored by load_checkpoint, applied at the next bind
        self._frozen_fp = None
        self._train_fp = None  # version fingerprint of the trainable T5 right after a klab FusedAdam step (bf16 copies current)
        self._fwd_token = 0
        self._loss_options = {"label_smoothing": 0.0, "z_loss": 0.0}
        self._distill_options = {"distill_alpha": 0.0, "distill_temperature": 1.0}
        self._weight_norm = "sum"  # normaliser of a weighted loss: "sum" of the weights or "count" of the scored tokens
        self._loss_weights_next = None  # this call's target_encoding["loss_weights"], taken by _LossFn.forward
        self._teacher_next = None  # this call's target_encoding["teacher_logits"], taken by _LossFn.forward
        self._token_losses_valid = False  # the engine's per-token losses are those of a loss forward of this binding
        self._token_kl_valid = False  # ... and its per-token kl those of a distillation forward
        self._logits_valid = False  # the engine's logits buffer holds the logits of the last loss forward (it wrote no gradient)
        self._token_losses_shape = None  # ... and the shape of that forward's labels: [B, Lt] or [B, n, Lt]
        import weakref
        for p in self.transformer.parameters():  # lets klab_multimodalmodel_amd.optim.FusedAdam find its engine
            p._klab_owner = weakref.ref(self)

    # ---- weights -----------------------------------------------------------------------------
    @staticmethod
    def _load_tree(tree, sd):
        own = tree.state_dict()
        missing = [k for k in own if k not in sd and k not in tree._tied]
        if "shared.weight" not in sd and "encoder.embed_tokens.weight" in sd:
            sd = dict(sd)
            sd["shared.weight"] = sd["encoder.embed_tokens.weight"]
            missing = [k for k in missing if k != "shared.weight"]
        if missing:
            raise RuntimeError(f"Missing key(s) in state_dict: {missing[:5]}{'...' if len(missing) > 5 else ''}")
        with torch.no_grad():
            for k, p in tree.named_parameters():
                if k in sd:
                    if tuple(sd[k].shape) != tuple(p.shape):
                        raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(sd[k].shape)} vs model {tuple(p.shape)}")
                    p.copy_(sd[k].to(torch.float32))

    def _apply(self, fn, *a, **k):  # .to()/.cuda() replace parameter storage => rebind lazily
        self._bound_key = None
        return super()._apply(fn, *a, **k)

    def train(self, mode: bool = True):
        # nn.Module.train() would flip the frozen towers too; DDP(model) / model.train() callers expect the
        # reference's effective behaviour only if they call it -- train.py never does (ref/train.py:52 toggles
        # .transformer only).  Keep torch semantics: propagate, but Swin / language encoder have no train-mode ops here.
        return super().train(mode)

    # ---- engine plumbing ---------------------------------------------------------------------
    def _trainable(self):
        ps = list(self.transformer.ordered())
        if self.args.image_model_train:
            ps += list(self.image_model.ordered())
        return [p for p in ps if p.requires_grad]

    def _engine_for(self, pixels, src, tgt):
        B, Ls = src.shape
        # [B, n, Lt]: n captions per image, image-major rows on the decoder side of the binding; [B, Lt] binds as n = 1
        n, Lt = (tgt.shape[1], tgt.shape[2]) if tgt.dim() == 3 else (1, tgt.shape[1])
        dev = pixels.device
        if dev.type != "cuda":
            raise RuntimeError("klab MyModel runs on an MI355X (cuda/HIP device) only; there is no CPU fallback")
        key = (B, Ls, Lt, dev, n)
        if self._bound_key != key:
            eng = self._engine
            tensors = {"swin": [p.data for p in self.image_model.ordered()], "lang": [p.data for p in self.language_model.ordered()],
                       "main": [p.data for p in self.transformer.ordered()]}
            for ts in tensors.values():
                for t in ts:
                    if t.device != dev:
                        raise RuntimeError(f"Expected all tensors to be on the same device, but found {t.device} and {dev}")
            if "main" not in self._flat or self._flat["main"].device != dev:
                self._flat["main"] = torch.zeros(eng.grad_elems["main"], device=dev)
                self._flat["swin"] = torch.zeros(max(eng.grad_elems["swin"], 8), device=dev) if self.args.image_model_train else None
                self._views = None
            eng.bind(B, Ls, Lt, tensors, self._flat["main"], self._flat["swin"], dev, n=n)
            eng.set_graph(self.use_graph)
            if self._pending_rng is not None:  # load_checkpoint before the first forward: continue the saved dropout stream
                eng.set_rng(*self._pending_rng)
                self._pending_rng = None
            self._bound_key = key
            self._frozen_fp = None
            self._train_fp = None
            self._token_losses_valid = self._token_kl_valid = self._logits_valid = False
            if self._lora is not None:  # (the engine keeps the registration across re-binds; a moved model gets a new table)
                self._lora._install()
        return self._engine

    def _note_optimizer_step(self):
        """called by optim.FusedAdam: the step kernel rewrote the masters AND their compute-dtype copies."""
        self._train_fp = sum(p._version for p in self.transformer.parameters())
        if self._lora is not None:  # the copies are those of the bare masters now: the next forward casts and merges again
            self._lora._fp = None

    def _trainable_current(self):
        """True when nothing wrote the trainable T5 since the last fused optimizer step (tensor version counters) and the
        engine was not re-bound: the forward may then skip its fp32 -> bf16 weight cast.  With LoRA adapters attached: when nothing
        wrote a base or an adapter parameter since the last loss forward of this binding (the arena holds W + s B A of exactly
        these versions); otherwise the engine casts and then merges."""
        if self._lora is not None:
            return self._lora._current()
        if self._train_fp is None:
            return False
        if sum(p._version for p in self.transformer.parameters()) != self._train_fp:
            self._train_fp = None
            return False
        return True

    def _frozen_unchanged(self):
        """True when no frozen-tower parameter was written since the previous forward (tensor version counters):
        the engine may then keep its bf16 copies and the Swin position-bias tables."""
        ps = list(self.language_model.parameters())
        if not self.args.image_model_train:
            ps += list(self.image_model.parameters())
        fp = sum(p._version for p in ps)
        same = fp == self._frozen_fp
        self._frozen_fp = fp
        return same

    def _grad_targets(self):
        if self._views is None:
            out = []
            for mname, tree in (("main", self.transformer), ("swin", self.image_model)):
                flat = self._flat.get(mname)
                if flat is None:
                    continue
                for spec, p in zip(self._engine.params[mname], tree.ordered()):
                    if spec.grad_off >= 0:
                        out.append((p, flat[spec.grad_off:spec.grad_off + p.numel()].view(p.shape), mname))
            self._views = out
        return [(p, v) for p, v, _m in self._views if p.requires_grad]

    # ---- loss options -------------------------------------------------------------------------
    def set_loss_options(self, label_smoothing=0.0, z_loss=0.0, distill_alpha=0.0, distill_temperature=1.0, weight_norm="sum"):
        """Options of the training loss, for every forward from now on (train and eval mode, with or without gradients; generate and
        score are not touched).  For each scored token with logits x, label y and lse = logsumexp(x):
            l = lse - (1 - label_smoothing) x_y - (label_smoothing / V) sum_j x_j + z_loss lse^2
        label_smoothing is torch.nn.functional.cross_entropy's (0 <= label_smoothing < 1), z_loss the coefficient of mesh-tensorflow
        T5's auxiliary z-loss (>= 0; T5, T5 v1.1 and Flan-T5 were pre-trained with 1e-4).  Per-token weights travel with the call
        instead: target_encoding["loss_weights"], a float [B, Lt] tensor on the model's device (finite; >= 0 under
        weight_norm="sum"), used for that forward only ([B, n, Lt] with labels [B, n, Lt]); the loss is sum w l / sum w over the tokens whose label is not -100.  With
        both options 0 and no weights the forward runs exactly the launches of the plain loss.
        These are hyper-parameters of the training script, not model state: save, state_dict and checkpoint.py do not store them.
        Under klab DDP every rank normalises by its own sum of weights, exactly as it normalises by its own count of scored tokens
        without them.
        Knowledge distillation: with distill_alpha in (0, 1] every loss forward needs target_encoding["teacher_logits"], a bf16 or
        fp32 tensor [B, Lt, V] ([B, n, Lt, V] with labels [B, n, Lt]) of FINITE teacher logits, contiguous and on the model's device,
        read in place by that forward's loss kernel and never copied (keep it alive and unchanged until the forward has run).  With
        T = distill_temperature (finite, > 0), p = softmax(t / T) and q = softmax(x / T) the token's loss becomes
            (1 - distill_alpha) l + distill_alpha T^2 KL(p || q)
        (Hinton's form: the T^2 keeps the soft term's gradient scale independent of T); tokens without a label add nothing to either
        term, weights and the normalisation are as above.  With distill_alpha == 0 a teacher is refused and every forward issues the
        launches it issues without this option.  distill.teacher_logits computes the tensor from a second MyModel.
        weight_norm: "sum" (the default) normalises a weighted loss by the sum of the weights, as above.  "count" makes it
            sum w l / N,   N = the number of tokens whose label is not -100,
        with d/dx = (w / N) [...]: the form for weights of either sign, such as the advantages of self-critical training
        (scst.SelfCritical), whose sum is near zero.  All-ones weights give the plain loss's bits under both; without weights and
        with neutral options "count" runs the plain launches.  Under klab DDP every rank divides by its own count."""
        eps, z = float(label_smoothing), float(z_loss)
        alpha, temp = float(distill_alpha), float(distill_temperature)
        if not (math.isfinite(eps) and 0.0 <= eps < 1.0):
            raise ValueError(f"`label_smoothing` has to be a finite float in [0, 1), but is {label_smoothing}")
        if not (math.isfinite(z) and z >= 0.0):
            raise ValueError(f"`z_loss` has to be a finite float >= 0, but is {z_loss}")
        if not (math.isfinite(alpha) and 0.0 <= alpha <= 1.0):
            raise ValueError(f"`distill_alpha` has to be a finite float in [0, 1], but is {distill_alpha}")
        if not (math.isfinite(temp) and temp > 0.0):
            raise ValueError(f"`distill_temperature` has to be a finite float > 0, but is {distill_temperature}")
        if weight_norm not in ("sum", "count"):
            raise ValueError(f"`weight_norm` has to be 'sum' or 'count', but is {weight_norm!r}")
        self._loss_options = {"label_smoothing": eps, "z_loss": z}
        self._distill_options = {"distill_alpha": alpha, "distill_temperature": temp}
        self._weight_norm = weight_norm

    @property
    def loss_options(self):
        """dict(label_smoothing, z_loss) as set_loss_options left them, and distill_alpha and distill_temperature beside them once
        either differs from its default (0 and 1): a model that never asked for distillation reads back the two options it always had.
        weight_norm is reported likewise, once it differs from 'sum'"""
        out = dict(self._loss_options)
        if self._distill_options != {"distill_alpha": 0.0, "distill_temperature": 1.0}:
            out.update(self._distill_options)
        if self._weight_norm != "sum":
            out["weight_norm"] = self._weight_norm
        return out

    def token_losses(self):
        """fp32 [B, Lt] device tensor ([B, n, Lt] after a forward on [B, n, Lt] labels): a copy of the per-token losses l of the last
        loss forward (unweighted, with the loss options of that forward -- under distillation the combined
        (1 - alpha) l + alpha T^2 kl; 0 where the label is -100).  sum w l / sum w over the scored tokens is the loss that forward
        returned."""
        if not self._token_losses_valid:
            raise RuntimeError("token_losses(): no loss forward has run on this binding yet (generate and score keep none)")
        return self._engine.buffer("loss_row").view(self._token_losses_shape).clone()

    def token_kl(self):
        """fp32 device tensor shaped like token_losses(): a copy of the per-token KL(softmax(t / T) || softmax(x / T)) of the last loss
        forward (unweighted, without the factor alpha T^2; 0 where the label is -100).  That forward must have had a teacher."""
        if not self._token_kl_valid:
            raise RuntimeError("token_kl(): the last loss forward on this binding had no target_encoding['teacher_logits'] "
                               "(or none has run yet; generate and score keep none)")
        return self._engine.buffer("kl_row").view(self._token_losses_shape).clone()

    def logits(self):
        """A VIEW [B, Lt, V] ([B, n, Lt, V] after a forward on [B, n, Lt] labels) of the engine's logits in the model's compute dtype,
        after a loss forward that wrote no gradient.  Valid until this model's next forward, generate or score: clone it to keep it."""
        if not self._logits_valid:
            raise RuntimeError("logits(): the engine holds no logits: no loss forward has run on this binding since the last generate or "
                               "score, or the last one replaced them in place by d loss / d logits (grad mode on with trainable "
                               "parameters).  Call the model under torch.no_grad() first")
        return self._engine.buffer("logits").view(*self._token_losses_shape, -1)

    def _check_teacher_alias(self, eng, teacher):
        own = eng.buffer("logits")
        a0, a1 = own.data_ptr(), own.data_ptr() + own.numel() * own.element_size()
        b0, b1 = teacher.data_ptr(), teacher.data_ptr() + teacher.numel() * teacher.element_size()
        if a0 < b1 and b0 < a1:
            raise ValueError(f"target_encoding['teacher_logits'] {tuple(teacher.shape)} {teacher.dtype} overlaps this model's own logits buffer "
                             "(a view from logits() of the same model?): the loss kernel rewrites that buffer while it reads the teacher; "
                             "pass a clone")

    def flat_grads(self, model="main"):
        return self._flat.get(model)

    def grad_norms(self, norm_type=2.0):
        """(names, norms) of the trainable parameters' gradients: HF state-dict names and the fp32 device tensor of their norms with
        the total norm last, from one multi-tensor launch and without a host read (optim.grad_norms)"""
        from ..optim import grad_norms
        return grad_norms(self, norm_type)

    # ---- the reference surface -----------------------------------------------------------------
    def forward(self, images, source_encoding, target_encoding=None, return_loss=True):
        self._join_pending_update()  # an in-backward optimizer update nobody joined through step()
        self._join_pending_reduce()  # nobody consumed the last backward's gradients through FusedAdam: join now
        pixels = images["pixel_values"]
        src = source_encoding["input_ids"]
        if pixels.dim() != 4 or pixels.shape[1] != self.swin_cfg.num_channels:
            raise ValueError("Make sure that the channel dimension of the pixel values match with the one set in the configuration.")
        if pixels.shape[2] != self.swin_cfg.image_size or pixels.shape[3] != self.swin_cfg.image_size:
            raise NotImplementedError(f"images must be {self.swin_cfg.image_size}x{self.swin_cfg.image_size} (the configured size)")
        pixels = pixels.to(torch.float32).contiguous()
        src = src.to(torch.int64).contiguous()
        if return_loss:
            tgt = target_encoding["input_ids"].to(torch.int64).contiguous()
            # n captions per image: labels [B, n, Lt] over the B images (one pass of the Swin tower and both encoders per image); the
            # loss is the 2-D call's on pixel_values / source ids repeat_interleave(n, 0) and the labels viewed [B*n, Lt] -- one mean
            # over the scored tokens of all captions.  A caption whose labels are all -100 (an image with fewer captions) adds nothing.
            grouped = tgt.dim() == 3
            if tgt.dim() not in (2, 3) or tgt.shape[0] != src.shape[0] or 0 in tgt.shape:
                raise ValueError(f"target_encoding['input_ids'] has to be [B, Lt] or [B, n, Lt] with B = {src.shape[0]} (the images) and "
                                 f"n >= 1 captions per image, got {tuple(tgt.shape)}")
            weights = target_encoding["loss_weights"] if "loss_weights" in target_encoding else None
            if weights is not None:
                if not torch.is_tensor(weights) or not weights.is_floating_point() or tuple(weights.shape) != tuple(tgt.shape):
                    raise ValueError(f"target_encoding['loss_weights'] has to be a float tensor {'[B, n, Lt] = ' if grouped else ''}"
                                     f"{tuple(tgt.shape)}, got "
                                     f"{getattr(weights, 'dtype', type(weights))} {tuple(getattr(weights, 'shape', ()))}")
                if weights.device != tgt.device:
                    raise ValueError(f"target_encoding['loss_weights'] {'[B, n, Lt] ' if grouped else ''}is on {weights.device}, "
                                     f"the labels on {tgt.device}")
                weights = weights.detach().to(torch.float32).contiguous()
            teacher = target_encoding["teacher_logits"] if "teacher_logits" in target_encoding else None
            alpha = self._distill_options["distill_alpha"]
            if teacher is not None:
                want = tuple(tgt.shape) + (self.main_cfg.vocab_size,)
                if not torch.is_tensor(teacher) or teacher.dtype not in (torch.bfloat16, torch.float32) or tuple(teacher.shape) != want:
                    raise ValueError(f"target_encoding['teacher_logits'] has to be a bfloat16 or float32 tensor "
                                     f"{'[B, n, Lt, V] = ' if grouped else '[B, Lt, V] = '}{want}, got "
                                     f"{getattr(teacher, 'dtype', type(teacher))} {tuple(getattr(teacher, 'shape', ()))}")
                if teacher.device != pixels.device:
                    raise ValueError(f"target_encoding['teacher_logits'] {tuple(teacher.shape)} is on {teacher.device}, the model's inputs on "
                                     f"{pixels.device}")
                if not teacher.is_contiguous():
                    raise ValueError(f"target_encoding['teacher_logits'] {tuple(teacher.shape)} with strides {tuple(teacher.stride())} is not "
                                     "contiguous (it is read in place, never copied)")
                if alpha == 0.0:
                    raise ValueError(f"target_encoding['teacher_logits'] {tuple(teacher.shape)} was given, but distill_alpha is 0: call "
                                     "set_loss_options(distill_alpha=...) first or leave the teacher out")
                teacher = teacher.detach()
            elif alpha > 0.0:
                raise ValueError(f"distill_alpha is {alpha}, but target_encoding has no 'teacher_logits' for this loss forward")
            self._loss_weights_next = weights
            self._teacher_next = teacher
            params = self._trainable()
            if self._lora is not None:  # behind the base parameters: the loss has a grad_fn although the base T5 is frozen
                params = params + [p for p in self._lora.parameters()]
            # (grad mode is off inside Function.forward, so decide here whether d logits must be produced)
            want_grad = torch.is_grad_enabled() and any(p.requires_grad for p in params)
            return _LossFn.apply(self, want_grad, pixels, src, tgt, *params)
        return self.generate(pixels, src)

    @torch.no_grad()
    def generate(self, pixels, src, max_length=20, kv_cache=True, num_beams=1, length_penalty=1.0, early_stopping=False,
                 num_return_sequences=1, return_scores=False, do_sample=False, temperature=1.0, top_k=50, top_p=1.0,
                 repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None, min_length=0, min_new_tokens=None,
                 return_logprobs=False, best_of=None, decoder_input_ids=None, constraint=None, constraint_set=None,
                 return_cross_attention=False):
        """greedy decoding with HF's default generation settings (ref/models/model.py:28: max_length 20, no sampling).
        Every kv_cache=True call is one decoding session on the device (_generate_on_device; SURVEY §8 row f-3, HF/t5:308-332):
        prefill = one evaluation-mode forward (Swin, both encoders, the cross K/V of all layers, decoder position 0), then every
        further token runs the decoder over ONE new position against the session's per-layer K/V cache and chooses the next token
        on the device; the host reads one stop word per step.  Plain greedy decoding is the "pick" session without processors.
        kv_cache=False (greedy without processors only) is the independent cross-check of the cache: a host loop that re-runs
        decoder + LM head over the whole prefix per token.
        num_beams > 1: HF's beam search (`_beam_search`, `generate(num_beams=...)`) -- see _generate_beam.
        do_sample=True: HF's `_sample` with temperature -> top-k -> top-p -- see _generate_sample.
        repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_length, min_new_tokens: HF's logits processors with HF's
        names, defaults and checks (logits_proc.logits_processor_settings), in front of all three loops as in HF: on the fp32
        logits for greedy and sampling (before the warpers), on log_softmax(logits) for beam search; the history is the decoder
        sequence with its start token.  One `klab_logits_process_rows` per step (csrc/logits_proc.hip); in a pick session it also
        takes the arg-max (lowest id among ties, as torch.argmax), pads finished rows and sets the stop word.
        Limit: sampling, pick and beam search with processors need vocab_size <= 32768 (the register row of
        klab_logits_process_rows; every supported T5 checkpoint has 32100-32128) and raise ValueError above it, plain greedy
        decoding included; a session also needs max_length >= 2.  kv_cache=False has neither limit.
        return_logprobs=True (greedy and sampling on the K/V cache): returns (sequences, info) with info["token_logprobs"]
        [rows, L] fp32 -- HF's transition score log_softmax(s)[token] of every generated token, s the processed scores the step
        chose from (greedy: after the processors; sampling: after processors, temperature, top-k and top-p), written by the
        choosing kernel itself; column 0 (the start token) and everything after a row's EOS are 0 -- info["lengths"] [rows] int32
        (generated tokens through the first EOS) and info["scores"] [rows] = sum of the row's log-probabilities /
        lengths ** length_penalty, beam search's convention.
        best_of=N (sampling only, num_return_sequences <= N <= 64): draws N rows per image and returns the num_return_sequences
        best by that score, best first, chosen and gathered on the device (klab_gen_finalize).
        decoder_input_ids (int64 [B, P]; greedy and sampling on the K/V cache, with or without processors): HF's decoder prompt.
        The start token is prepended unless column 0 already is the start token in some row (HF's
        `_prepare_decoder_input_ids_for_generation`); each image's prompt is shared by its num_return_sequences rows; the session
        takes the prompt positions from a table (klab_force_rows, no logits read) and chooses the rest as without one.  As in HF
        max_length counts the prompt, the processors see it as history (min_new_tokens counts from its end) and an EOS inside it
        does not finish the row.  Not with num_beams > 1, kv_cache=False, return_logprobs or best_of.
        return_cross_attention=True (greedy and sampling on the K/V cache, with or without processors, best_of or a decoder
        prompt): returns (sequences, info) with info["cross_attention"] fp32 [rows, n_dec_layers, L, Le] -- HF's
        `cross_attentions` of output_attentions=True averaged over the heads: [r, i, p] is layer i's attention over the encoder
        tokens that produced row r's token of position p (the query of position p - 1), written by the session itself
        (klab_t5_decode_attn_map beside every cross-attention of the decoder; tokens and log-probabilities are bit-identical with
        and without it).  The Le encoder tokens are the info["image_tokens"] Swin tokens, an info["image_grid"] = (g, g) raster,
        followed by the source-text tokens (the reference's torch.cat order).  Column 0 (the start token) and everything after a
        row's EOS are 0; with best_of the rows are those of the sequences.  With return_logprobs as well the same info carries
        both.  Not with num_beams > 1 (beam search re-parents its rows every step) or kv_cache=False.
        constraint (a constrain.TokenTrie on the model's device, built for this vocabulary and EOS): decoding into a closed set of
        phrases, HF's `prefix_allowed_tokens_fn` without the callback -- every row may only choose a child of the trie node it
        stands on, a finished phrase or a row off the trie only EOS (klab_constrain_rows, one launch more per position).  Greedy
        decoding returns the arg-max phrase at every branch, num_beams > 1 the best phrases of a set of any size with their
        scores.  Works with sampling, all processors, return_logprobs / best_of (the log-probabilities are those of the masked
        scores, renormalised over the allowed tokens for greedy and sampling), return_cross_attention and decoder_input_ids (the
        phrase starts behind the prompt; the prompt is not walked).  constraint_set (int [B] tensor or list, default 0): the
        phrase set of every image for a trie of several (TokenTrie.from_sequence_sets).  Needs kv_cache=True and vocab_size <=
        32768.  Not checked: processors that ban everything the trie allows leave a row of -inf, which picks token 0."""
        roots = self._constraint_roots(constraint, constraint_set, src, kv_cache)
        if return_cross_attention:
            if num_beams > 1:
                raise ValueError("return_cross_attention needs num_beams == 1 (beam search re-parents its rows every step and keeps no maps)")
            if not kv_cache:
                raise ValueError("return_cross_attention runs on the K/V cache only: it needs kv_cache=True")
        prompt = None
        if decoder_input_ids is not None:
            for bad, why in ((num_beams > 1, "num_beams > 1 (beam search takes no forced tokens)"),
                             (not kv_cache, "kv_cache=False (the prompt is forced inside the K/V-cache session)"),
                             (return_logprobs, "return_logprobs (an EOS inside the prompt would end the row's score)"),
                             (best_of is not None, "best_of (an EOS inside the prompt would end the row's score)")):
                if bad:
                    raise ValueError(f"decoder_input_ids is not supported with {why}")
            prompt = self._decoder_prompt(decoder_input_ids, src.shape[0], max_length)
        if return_logprobs or best_of is not None:
            what = "return_logprobs" if return_logprobs else "best_of"
            if num_beams > 1:
                raise ValueError(f"{what} needs num_beams == 1 (beam search returns its own scores: return_scores=True)")
            if not kv_cache:
                raise ValueError(f"{what} runs on the K/V cache only: it needs kv_cache=True")
        if best_of is not None:
            if not do_sample:
                raise ValueError("best_of ranks sampled sequences: it needs do_sample=True")
            if not isinstance(best_of, int) or best_of < num_return_sequences:
                raise ValueError(f"`best_of` ({best_of}) has to be an integer greater or equal to `num_return_sequences` "
                                 f"({num_return_sequences})")
            if best_of > 64:
                raise ValueError(f"`best_of` ({best_of}) has to be at most 64")
        procs = logits_processor_settings(repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_length, min_new_tokens,
                                          eos_token_id=self.main_cfg.eos_token_id, vocab_size=self.main_cfg.vocab_size,
                                          prompt_length=1 if prompt is None else prompt.shape[1])
        if do_sample:
            if num_beams > 1:
                raise NotImplementedError("beam sampling (do_sample=True with num_beams > 1) is not supported")
            if not kv_cache:
                raise ValueError("sampling runs on the K/V cache only: do_sample=True needs kv_cache=True")
            if return_scores:
                raise ValueError("return_scores needs num_beams > 1 (sampling keeps no sequence scores)")
            if not isinstance(temperature, (int, float)) or not temperature > 0:
                raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive float, otherwise your next token "
                                 "scores will be invalid.")
            if not isinstance(top_k, int) or top_k < 0:
                raise ValueError(f"`top_k` has to be a non-negative integer (0 disables it), but is {top_k}")
            if not isinstance(top_p, (int, float)) or top_p < 0 or top_p > 1.0:
                raise ValueError(f"`top_p` has to be a float > 0 and < 1, but is {top_p}")
            if num_return_sequences < 1:
                raise ValueError(f"`num_return_sequences` has to be a positive integer, but is {num_return_sequences}")
            return self._generate_sample(pixels, src, max_length, num_return_sequences, float(temperature), int(top_k), float(top_p),
                                         procs, return_logprobs=return_logprobs, best_of=best_of, length_penalty=length_penalty,
                                         prompt=prompt, return_cross_attention=return_cross_attention, constraint=roots)
        if num_return_sequences > num_beams:
            raise ValueError(f"`num_return_sequences` ({num_return_sequences}) has to be smaller or equal to `num_beams` ({num_beams}).")
        if num_beams > 1:
            if not kv_cache:
                raise ValueError("beam search runs on the K/V cache only: kv_cache=False needs num_beams=1")
            return self._generate_beam(pixels, src, max_length, num_beams, length_penalty, early_stopping, num_return_sequences,
                                       return_scores, procs, constraint=roots)
        if return_scores:
            raise ValueError("return_scores needs num_beams > 1 (greedy decoding keeps no sequence scores)")
        if kv_cache:
            return self._generate_sample(pixels, src, max_length, 1, 1.0, 0, 1.0, procs, pick=True, return_logprobs=return_logprobs,
                                         length_penalty=length_penalty, prompt=prompt, return_cross_attention=return_cross_attention,
                                         constraint=roots)
        if procs is not None:
            raise ValueError("logits processors run on the K/V cache only: repetition_penalty, no_repeat_ngram_size, bad_words_ids, "
                             "min_length and min_new_tokens need kv_cache=True")
        B = src.shape[0]
        cfg = self.main_cfg
        steps = max_length - 1
        tgt = torch.full((B, steps), cfg.pad_token_id, dtype=torch.int64, device=src.device)
        done = torch.zeros(B, dtype=torch.bool, device=src.device)
        was_training = self.transformer.training
        self.transformer.eval()
        try:
            eng = self._engine_for(pixels, src, tgt)
            self._token_losses_valid = self._token_kl_valid = self._logits_valid = False  # (these forwards score a pad target ...
            eng.set_loss_options()                # ... with the plain loss: the launches generate always issued)
            for t in range(steps):
                eng.forward(pixels, src, tgt, training=(8 if t > 0 else 0) | (2 if t > 0 else 0), seed=self._seed_base, want_grad=False)
                nxt = eng.buffer("logits").view(B, steps, -1)[:, t].float().argmax(-1)
                nxt = torch.where(done, torch.full_like(nxt, cfg.pad_token_id), nxt)
                tgt[:, t] = nxt
                done |= nxt == cfg.eos_token_id
                if bool(done.all()):
                    tgt = tgt[:, :t + 1]
                    break
        finally:
            self.transformer.train(was_training)
        start = torch.full((B, 1), cfg.decoder_start_token_id, dtype=torch.int64, device=src.device)
        return torch.cat([start, tgt], dim=1)

    def _constraint_roots(self, constraint, constraint_set, src, kv_cache):
        """generate's constraint, checked before anything touches the device: (trie, the start node of every image as a host int32
        [B] tensor), or None without one"""
        from ..constrain import TokenTrie
        if constraint is None:
            if constraint_set is not None:
                raise ValueError("constraint_set names the phrase sets of a trie: it needs `constraint`")
            return None
        cfg = self.main_cfg
        B = src.shape[0]
        if not isinstance(constraint, TokenTrie):
            raise ValueError(f"`constraint` has to be a constrain.TokenTrie, got {type(constraint).__name__}")
        if constraint.vocab_size != cfg.vocab_size or constraint.eos_token_id != cfg.eos_token_id:
            raise ValueError(f"the trie was built for vocab_size {constraint.vocab_size} / eos_token_id {constraint.eos_token_id}, the "
                             f"model has {cfg.vocab_size} / {cfg.eos_token_id}")
        if constraint.device != src.device:
            raise ValueError(f"the trie is on {constraint.device}, the batch on {src.device}: move it with trie.to(device)")
        if not kv_cache:
            raise ValueError("constrained decoding runs on the K/V cache only: `constraint` needs kv_cache=True")
        which = torch.zeros(B, dtype=torch.int64) if constraint_set is None else torch.as_tensor(constraint_set).cpu()
        if which.dim() != 1 or which.shape[0] != B or which.dtype.is_floating_point or which.dtype == torch.bool:
            raise ValueError(f"constraint_set has to be an integer tensor or list [{B}], got {which.dtype} {tuple(which.shape)}")
        if int(which.min()) < 0 or int(which.max()) >= constraint.n_sets:
            raise ValueError(f"constraint_set names sets outside the {constraint.n_sets} of the trie")
        return constraint, constraint.roots.cpu()[which.long()].to(torch.int32)

    def _decoder_prompt(self, decoder_input_ids, B, max_length):
        """HF's decoder prompt [B, Lp] on the host, start token first, from generate's decoder_input_ids (checked before anything
        touches the device); its ids must be the model's"""
        cfg = self.main_cfg
        ids = torch.as_tensor(decoder_input_ids)
        if ids.dim() != 2 or ids.shape[0] != B or ids.shape[1] < 1 or ids.dtype != torch.int64:
            raise ValueError(f"decoder_input_ids has to be an int64 tensor [{B}, P] with P >= 1, got {ids.dtype} {tuple(ids.shape)}")
        ids = ids.cpu()
        if int(ids.min()) < 0 or int(ids.max()) >= cfg.vocab_size:
            raise ValueError(f"decoder_input_ids holds ids outside [0, {cfg.vocab_size})")
        first = ids[:, 0] == cfg.decoder_start_token_id
        if not bool(first.any()):  # HF prepends the start token unless some row already begins with it
            ids = torch.cat([torch.full((B, 1), cfg.decoder_start_token_id, dtype=torch.int64), ids], 1)
        elif not bool(first.all()):
            raise ValueError("decoder_input_ids: column 0 is the start token in some rows only; every row of a session starts from "
                             "the start token, so give it in all rows or in none")
        if ids.shape[1] >= max_length:
            raise ValueError(f"Input length of decoder_input_ids is {ids.shape[1]}, but `max_length` is set to {max_length}. This can "
                             "lead to unexpected behavior. You should consider increasing `max_length` or, better yet, setting "
                             "`max_new_tokens`.")
        return ids

    @torch.no_grad()
    def score(self, pixels, src, candidates, length_penalty=1.0, top=None, return_cross_attention=False):
        """How likely each of N given captions is for each image: candidates int64 [B, N, L] as labels are (no start token, each
        row closed by EOS, whatever follows the first EOS ignored; a row without EOS counts all L tokens), 1 <= N <= 64, L >= 1.
        One prefill at B rows, then ONE force session of B*N rows against the shared cross K/V (Swin and both encoders run once per
        image, not once per candidate): every position's token comes from the candidates (klab_force_rows), which also writes
        log_softmax(logits)[token]; the L - 1 decoder steps are enqueued without a host read, then one klab_gen_finalize.
        Returns dict(token_logprobs [B, N, L] fp32, 0 after a row's EOS; lengths [B, N] int32, tokens through the first EOS;
        scores [B, N] = sum / lengths ** length_penalty, the convention of generate's info["scores"] (length_penalty=0: the
        sequence log-likelihood); order [B, top or N] int64, each image's candidate indices best first, ranked on the device).
        return_cross_attention=True adds cross_attention fp32 [B, N, n_dec_layers, L, Le]: [b, j, i, l] is layer i's head-mean
        attention over the encoder tokens (image tokens first, see generate) that predicted label l of candidate j, 0 after the
        row's first EOS; with it image_tokens and image_grid.  The other entries are bit-identical with and without it."""
        cfg = self.main_cfg
        cand = torch.as_tensor(candidates)
        if cand.dim() != 3 or cand.dtype != torch.int64:
            raise ValueError(f"candidates has to be an int64 tensor [B, N, L], got {cand.dtype} {tuple(cand.shape)}")
        B, N, L = cand.shape
        if B != src.shape[0]:
            raise ValueError(f"candidates holds {B} images, the batch {src.shape[0]}")
        if N < 1 or N > 64:
            raise ValueError(f"candidates per image ({N}) has to be between 1 and 64")
        if L < 1:
            raise ValueError("candidates need at least one token")
        if top is not None and (not isinstance(top, int) or top < 1 or top > N):
            raise ValueError(f"`top` ({top}) has to be an integer between 1 and the number of candidates ({N})")
        if int(cand.min()) < 0 or int(cand.max()) >= cfg.vocab_size:
            raise ValueError(f"candidates holds ids outside [0, {cfg.vocab_size})")
        dev = src.device
        pixels = pixels.to(torch.float32).contiguous()
        src = src.to(torch.int64).contiguous()
        # the session's table: column p is position p (column 0, the start token's, is not read)
        table = torch.cat([torch.full((B * N, 1), cfg.decoder_start_token_id, dtype=torch.int64, device=dev),
                           cand.to(dev).reshape(B * N, L)], 1).contiguous()
        tgt = torch.full((B, L), cfg.pad_token_id, dtype=torch.int64, device=dev)
        was_training = self.transformer.training
        self.transformer.eval()
        try:
            eng = self._engine_for(pixels, src, tgt)
            self._token_losses_valid = self._token_kl_valid = self._logits_valid = False  # (this forward scores a pad target ...
            eng.set_loss_options()                # ... with the plain loss: the launches generate and score always issued)
            eng.forward(pixels, src, tgt, training=0, seed=self._seed_base, want_grad=False)
            gen = eng.gen_cfg("force", N, L + 1, cfg.eos_token_id, cfg.pad_token_id, want_logprobs=True)
            nbytes = eng.gen_workspace_bytes(gen)
            if nbytes == 0:
                raise ValueError(f"scoring: unsupported candidates per image {N} / length {L} for this model")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            eng.gen_set_forced(table, L)
            att = self._attn_maps_for(eng, gen, B * N, L + 1) if return_cross_attention else None
            eng.gen_begin(gen, ws)
            for t in range(1, L):  # nothing is chosen: the host has nothing to wait for
                eng.gen_step(t, ws)
            lp, scores, lens, order = eng.gen_scores(ws, L + 1, N if top is None else top, length_penalty)
        finally:
            self.transformer.train(was_training)
        order = order.long().view(B, -1) - torch.arange(B, device=dev).view(B, 1) * N
        out = dict(token_logprobs=lp[:, 1:].reshape(B, N, L), lengths=lens.view(B, N), scores=scores.view(B, N), order=order)
        if return_cross_attention:  # label l is session column l + 1
            out.update(self._attn_info(att[:, :, 1:].permute(1, 0, 2, 3).reshape(B, N, att.shape[0], L, -1)))
        return out

    def _generate_on_device(self, pixels, src, max_length, mode, n, procs=None, num_return_sequences=None, temperature=1.0, top_k=0,
                            top_p=1.0, length_penalty=1.0, early_stopping=False, logprobs=False, prompt=None, maps=False,
                            constraint=None):
        """One prefill at B rows (Swin, both encoders and the cross K/V run once per image, not per row), then a decoding session of
        B*n rows on the device (row b*n + j: beam / sample j of image b, HF's `_expand_inputs_for_generation`): every step is the
        decoder over B*n rows and the mode's choice of the next tokens (`klab_engine_gen_step`); the host reads one stop word per
        step.  mode "beam": HF's `_beam_search` with n = num_beams, returning num_return_sequences hypotheses per image (start
        token, pads after EOS, cropped to the longest returned one) and their scores.  "sample": HF's `_sample` with n =
        num_return_sequences; the draws come from a counter hash of one 64-bit seed taken from torch's default CPU generator per
        call (torch.manual_seed reproduces a call).  "pick": greedy decoding, the processed arg-max instead of a draw (no seed is
        taken).  Sampling and pick return [B*n, L] int64 (start token, pad after EOS, cropped when every row is done) and None.
        procs: the logits processors' settings (logits_proc.logits_processor_settings), None = none.
        logprobs (sampling and pick): the session keeps every chosen token's log-probability and the second value returned is
        info = dict(token_logprobs, scores, lengths) (see generate); with num_return_sequences < n the rows returned are each
        image's num_return_sequences best by score, best first, ranked and gathered on the device.
        prompt (sampling and pick): the decoder prompt [B, Lp] with its start token (_decoder_prompt); its Lp - 1 tokens after
        the start token are forced at positions 1 .. Lp - 1 of each image's n rows.
        maps (sampling and pick): the session also writes its cross-attention maps (Engine.gen_set_attn) and info carries
        cross_attention [rows, n_dec_layers, L, Le], image_tokens and image_grid (see generate), for the rows returned.
        constraint: (trie, host roots [B]) of _constraint_roots; the session walks and applies the trie itself."""
        if mode == "beam" and early_stopping not in (False, True, "never"):
            raise ValueError(f"early_stopping must be False, True or 'never', got {early_stopping!r}")
        if max_length < 2:
            raise ValueError("max_length must count the start token and at least one generated token")
        B = src.shape[0]
        cfg = self.main_cfg
        n = int(n)
        seed = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (), dtype=torch.int64)) if mode == "sample" else 0
        # beam search's fill value of unfinished positions is HF's `pad_token_id or eos_token_id` (a pad id of 0 yields to EOS)
        pad = (cfg.pad_token_id or cfg.eos_token_id) if mode == "beam" else cfg.pad_token_id
        tgt = torch.full((B, max_length - 1), cfg.pad_token_id, dtype=torch.int64, device=src.device)
        was_training = self.transformer.training
        self.transformer.eval()
        try:
            eng = self._engine_for(pixels, src, tgt)
            self._token_losses_valid = self._token_kl_valid = self._logits_valid = False  # (this forward scores a pad target ...
            eng.set_loss_options()                # ... with the plain loss: the launches generate and score always issued)
            eng.forward(pixels, src, tgt, training=0, seed=self._seed_base, want_grad=False)
            if constraint is not None:
                constraint = (constraint[0], constraint[1].to(src.device).contiguous())
            gen = eng.gen_cfg(mode, n, max_length, cfg.eos_token_id, pad, temperature, top_k, top_p, seed, length_penalty, early_stopping,
                              procs, want_logprobs=logprobs, constraint=constraint)
            nbytes = eng.gen_workspace_bytes(gen)
            if nbytes == 0:
                what = {"beam": f"beam search: unsupported num_beams={n}", "sample": f"sampling: unsupported num_return_sequences={n}",
                        "pick": f"greedy decoding on the K/V cache: unsupported vocab_size={cfg.vocab_size}"}[mode]
                raise ValueError(f"{what} / max_length={max_length} for this model")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
            if prompt is not None and prompt.shape[1] > 1:
                eng.gen_set_forced(prompt.to(src.device).repeat_interleave(n, 0).contiguous(), prompt.shape[1] - 1)
            att = self._attn_maps_for(eng, gen, B * n, max_length) if maps else None
            eng.gen_begin(gen, ws)
            cur = 1
            while cur < max_length - 1 and eng.gen_going(ws, cur):
                eng.gen_step(cur, ws)
                cur += 1
            if mode != "beam":
                seq = eng.gen_result(ws, n, cur + 1)[0]
                if not logprobs and not maps:
                    return seq, None
                info, order = {}, None
                if logprobs:
                    n_out = num_return_sequences if num_return_sequences is not None and num_return_sequences < n else None
                    lp, scores, lens, order = eng.gen_scores(ws, cur + 1, n_out, length_penalty)
                    if order is not None:
                        order = order.long()
                        seq, lp, scores, lens = seq[order], lp[order], scores[order], lens[order]
                    info.update(token_logprobs=lp, scores=scores, lengths=lens)
                if maps:
                    att = att[:, :, :cur + 1].permute(1, 0, 2, 3)  # [B*n, n_dec_layers, L, Le]
                    info.update(self._attn_info(att[order] if order is not None else att.contiguous()))
                return seq, info
            seq, scores, lens = eng.gen_result(ws, num_return_sequences, max_length)
        finally:
            self.transformer.train(was_training)
        return seq[:, :1 + int(lens.max())], scores

    def _attn_maps_for(self, eng, gen, rows, max_length):
        """arms the cross-attention maps of the next gen_begin: f32 [n_dec_layers, rows, max_length, Le], the session's to clear and fill"""
        nbytes = eng.gen_attn_bytes(gen)
        if nbytes == 0:
            raise ValueError("cross-attention maps: these generation settings carry none")
        att = torch.empty(nbytes // 4, dtype=torch.float32, device=eng.workspace.device)
        eng.gen_set_attn(att)
        return att.view(self.main_cfg.num_decoder_layers, rows, max_length, -1)

    def _attn_info(self, att):
        """the cross-attention entries of a result: the maps and where the image tokens lie in their last dimension"""
        n_img = self._engine.n_img
        g = math.isqrt(n_img)
        return dict(cross_attention=att, image_tokens=n_img, image_grid=(g, g))

    def _generate_beam(self, pixels, src, max_length, num_beams, length_penalty, early_stopping, num_return_sequences, return_scores,
                       procs=None, constraint=None):
        """HF's `_beam_search` as a decoding session (_generate_on_device): the sequences, and their scores when return_scores"""
        seq, scores = self._generate_on_device(pixels, src, max_length, "beam", num_beams, procs, num_return_sequences,
                                               length_penalty=length_penalty, early_stopping=early_stopping, constraint=constraint)
        return (seq, scores) if return_scores else seq

    def _generate_sample(self, pixels, src, max_length, num_return_sequences, temperature, top_k, top_p, procs=None, pick=False,
                         return_logprobs=False, best_of=None, length_penalty=1.0, prompt=None, return_cross_attention=False,
                         constraint=None):
        """HF's `_sample` as a decoding session (_generate_on_device); pick=True: greedy decoding, the processed arg-max.
        return_logprobs / return_cross_attention: (sequences, info); best_of: that many rows per image, the num_return_sequences
        best returned"""
        n = num_return_sequences if best_of is None else best_of
        seq, info = self._generate_on_device(pixels, src, max_length, "pick" if pick else "sample", n, procs,
                                             num_return_sequences=num_return_sequences, temperature=temperature, top_k=top_k, top_p=top_p,
                                             length_penalty=length_penalty, logprobs=return_logprobs or best_of is not None,
                                             prompt=prompt, maps=return_cross_attention, constraint=constraint)
        if return_cross_attention and not return_logprobs:  # (best_of ranks by the scores; they were not asked for)
            info = {k: info[k] for k in ("cross_attention", "image_tokens", "image_grid")}
        return (seq, info) if return_logprobs or return_cross_attention else seq

    def _join_pending_update(self, device=None):
        """an optimizer update still running on its own stream (optim.FusedAdam(step_in_backward=True)) writes the weights:
        anything that reads them on the current stream (of `device`, default the current one) waits for it first"""
        if self._pending_opt_stream is not None:
            torch.cuda.current_stream(device).wait_stream(self._pending_opt_stream)
            self._pending_opt_stream = None

    def _join_pending_reduce(self):
        """klab DDP(overlap_optimizer=True) leaves the last backward's gradient all-reduces to whoever reads the gradients next:
        wait (stream-wise) for them and do the reducer's bookkeeping"""
        if self._pending_reduce is not None:
            red, self._pending_reduce = self._pending_reduce, None
            red.finish()

    def state_dict(self, *a, **k):
        self._join_pending_update()
        return super().state_dict(*a, **k)

    def save(self, result_name="best.pth"):
        self._join_pending_update()
        result_path = os.path.join(self.args.result_dir, result_name)
        checkpoints = {'transformer': self.transformer.state_dict()}
        if self.args.image_model_train:
            checkpoints['image_model'] = self.image_model.state_dict()
        torch.save(checkpoints, result_path)

    def load(self, result_name="best.pth"):
        result_path = os.path.join(self.args.result_dir, result_name)
        checkpoints = torch.load(result_path)
        self.transformer.load_state_dict(checkpoints['transformer'])
        if self.args.image_model_train:
            self.image_model.load_state_dict(checkpoints['image_model'])
