"""Drop-in `optim.Adam` / `optim.AdamW` / `optim.SGD` for the reference's UNCHANGED training loops (reference
mfm_mosi.py:403-404, 427-441):

    import factorized_amd.optim as optim                       # instead of: import torch.optim as optim
    from factorized_amd.mfm_model import MFM_KL_EF              # instead of: from mfm_model import MFM_KL_EF
    ...
    optimizer = optim.Adam(model.parameters())                  # :403, before model.to(device) as in the reference
    ...
    optimizer.zero_grad(); decoded, reg, missing = model.forward(batch_X); ...; loss.backward(); optimizer.step()

Every class here is a `torch.optim.Optimizer` (so `ReduceLROnPlateau(optimizer, 'min')`, `param_groups[0]['lr']`, `zero_grad()`
work as in the reference) built on one base, `_FlatOptimizer`, which holds everything that does not depend on the update rule.
Parameters that belong to a model with the fused engine (`MFM_KL_EF`, `MFM_KL`, `MFM`: every nn.Parameter is a view into ONE
flat buffer) and whose `.grad`s are the views of the model's flat gradient buffer (what `MFM_KL_EF`'s backward leaves behind)
take the flat path: ONE launch per model and step over the flat buffers.  Like torch, a parameter without a gradient is skipped
with all its state; tensors with a gradient become spans of the launch (adjacent tensors whose hyper-parameters and step counts
agree merge).  Everything else (other modules, models on the composed autograd path) goes through an inner stock torch
optimizer with the same hyper-parameters, and state moves between the two.  `torch.optim.Adam` itself keeps working too -- it is
just host-bound (78 tensors per step); see INTEGRATION.md for the measured step times.

`Adam` takes every option of torch.optim.Adam (weight decay, decoupled decay, AMSGrad, maximize; several parameter groups with
their own values) and `AdamW` derives from it as torch's does.  The reference's call -- no option, one group -- is ONE launch of
`mfm_adam_flat` (`mfm_adam_flat_spans` when some tensors received no gradient); any option goes to
`mfm_adam_ext_flat_spans_guarded` (see the class).  `SGD` is the reference's other optimizer line
(`optim.SGD(model.parameters(), lr=config["lr"], momentum=config["momentum"])`, mfm_mosi.py:404): `mfm_sgd_flat_spans_guarded`
with torch.optim.SGD's arithmetic and per-group hyper-parameters.

`zero_grad()` clears a fused model's flat gradient buffer with one launch and marks every tensor "no gradient yet" (= torch's
`set_to_none=True`: the next `step()` skips tensors the next backward does not reach) while leaving the `.grad` views attached;
`zero_grad(set_to_none=False)` keeps zero gradients in place, which is the reference's PyTorch-0.4 behaviour (a tensor that
once had a gradient keeps moving on its decaying first moment)."""
import ctypes as C
import warnings
import weakref

import numpy as np
import torch

from . import _flat, _lib
from ._flat import ptr as _ptr, stream_and_guard as _stream_and_guard      # (once per step: no attribute look-up)

ReduceLROnPlateau = torch.optim.lr_scheduler.ReduceLROnPlateau      # convenience: `optim.lr_scheduler` users import torch's
lr_scheduler = torch.optim.lr_scheduler
from . import swa_utils  # noqa: E402,F401  (`optim.swa_utils.AveragedModel`: torch's on any module, one launch between two fused models)


def _owner(p):
    from .mfm_model import _owner_of
    return _owner_of(p)


# Who may keep the in-launch hand-overs on is decided PER STEP by the optimizer that actually steps the model: a _FlatOptimizer
# marks the models it owns in every step(); any OTHER torch optimizer that steps parameters of a fused model -- an optimizer
# swap, an LR finder, per-stage optimizers built while the first one is still referenced -- takes the permission away before its
# update (a global step pre-hook: it knows nothing of the gradient guard and would apply a step whose hand-over gave up).
_FOREIGN = {}


def _foreign_step_hook(opt, args, kwargs):
    if isinstance(opt, _FlatOptimizer) or getattr(opt, "_mfm_inner", False):
        return
    key = id(opt)
    n = sum(len(g["params"]) for g in opt.param_groups)
    hit = _FOREIGN.get(key)
    if hit is None or hit[0] != n or hit[1]() is not opt:
        mods, seen = [], set()
        for g in opt.param_groups:
            for p in g["params"]:
                m = _owner(p)
                if m is not None and id(m) not in seen:
                    seen.add(id(m))
                    mods.append(weakref.ref(m))
        if len(_FOREIGN) > 64:
            _FOREIGN.clear()
        hit = _FOREIGN[key] = (n, weakref.ref(opt), mods)
    for r in hit[2]:
        m = r()
        if m is not None:
            m._guarded = False


import importlib as _il
_OPT_MOD = _il.import_module("torch.optim.optimizer")
_OPT_MOD.register_optimizer_step_pre_hook(_foreign_step_hook)
_GLOBAL_PRE, _GLOBAL_POST = _OPT_MOD._global_optimizer_pre_hooks, _OPT_MOD._global_optimizer_post_hooks


class _FlatOptimizer(torch.optim.Optimizer):
    """What `Adam` and `SGD` share: which fused models this optimizer owns, the step / zero_grad shell around one
    `_fused_step(model, group index of every tensor)` per owned model, the inner torch optimizer for everything that is not on
    the flat path, and the checkpoint format (torch's dict plus "fused" and "fallback").  A subclass supplies the update rule:
    its per-model state (`_stale`, `_new_state`, `_restore`, `_snapshot`, `_loaded_entry`), `_fused_step`, and how state moves
    to and from the inner optimizer (`_inner_rebuilt`, `_inner_stepping`)."""

    _inner_cls = None            # the stock torch optimizer behind _fallback, and the group keys it takes from ours
    _hyper = ()
    _state_word = "state"        # what the layout-mismatch error refuses to restart
    _capture_refusal = None      # message of the error step() raises inside a stream capture (None: capture is supported)

    def _init_flat(self):
        """(after torch's __init__) the state of the flat path; returns the owned models"""
        # module -> state of a fused model (weak keys: a model that is gone takes its optimizer state with it)
        self._fused = weakref.WeakKeyDictionary()
        self._fallback = None       # inner stock optimizer over everything that is not fused
        self._fallback_ids = None
        self._fm_key = None
        self._fm_list = []
        self._pending_fused = None  # fused states of a load_state_dict() waiting for their models' first step
        self._pending_fallback = None
        # this optimizer honours the gradient guard: the models it owns may run their in-launch hand-overs (a model under
        # any other optimizer stays on separate launches, mfm_model._FusedEngineMixin._guarded)
        return self._fused_models()

    def _fused_models(self):
        """[(model, group index of every tensor)] for the fused models whose parameters all lie in this optimizer's groups (the
        reference has one group: model.parameters()); cached while the groups hold the same lists of the same lengths"""
        key = tuple((id(g["params"]), len(g["params"]), id(g["params"][0]) if g["params"] else 0) for g in self.param_groups)
        if key == self._fm_key and all(r() is not None for r, _ in self._fm_list):
            return [(r(), gi) for r, gi in self._fm_list]
        gid = {}
        for k, g in enumerate(self.param_groups):
            for p in g["params"]:
                gid[id(p)] = k
        seen, out = set(), []
        for g in self.param_groups:
            for p in g["params"]:
                m = _owner(p)
                if m is None or id(m) in seen:
                    continue
                seen.add(id(m))
                if all(id(q) in gid for q in m._plist):
                    out.append((weakref.ref(m), np.array([gid[id(q)] for q in m._plist], dtype=np.int64)))
                    m._guarded = weakref.ref(self)
        self._fm_key, self._fm_list = key, out
        return [(r(), gi) for r, gi in out]

    # ------------------------------------------------------------------ the flat path
    def _flat_grads(self, m, eng):
        """the model's flat gradient buffer when this step can take the flat path, else None (the inner optimizer steps it)"""
        m._guarded = weakref.ref(self)          # (per step: the optimizer that steps the model answers for the guard)
        gflat = getattr(m, "_grad_flat", None)
        if gflat is None or not m._grad_views_attached():
            return None                      # gradients are ordinary per-tensor tensors
        if not m._fast_last:
            # a parameter was frozen / got a hook after fast-path steps: the flat path would move it (or skip everything);
            # hand the gradients back to per-tensor tensors and let the inner optimizer apply torch's rules
            m._detach_grad_views()
            return None
        if eng.poll_status():
            # a hand-over of this step (or an earlier one) gave up: its gradients carry the NaN guard, the guarded launch leaves
            # the parameters alone.  Clear the status, fall back to separate launches for the rest of the run, say so.
            eng.check_status(raise_on_error=False)
            warnings.warn(eng.status_message(), RuntimeWarning, stacklevel=4)      # (attributed to step())
        return gflat

    def _state_for(self, m, eng):
        st = self._fused.get(m)
        if st is None or self._stale(st, eng):
            st = self._new_state(eng)
            st["order"], st["extents"] = _flat.extents(eng.layout, padded=True)
            if self._pending_fused:                     # state restored by load_state_dict(), in the order it was saved
                self._restore(st, self._pending_fused.pop(0), eng)
            self._fused[m] = st
        return st

    def _require_fit(self, elements, tensors, eng, ok=True):
        if not (ok and elements == eng.layout.total and tensors == len(eng.layout.slots)):
            raise _lib.MfmError(
                "factorized_amd.optim.%s.load_state_dict: the saved fused state (%d elements, %d tensors) does not fit this "
                "model's flat layout (%d elements, %d tensors) -- a checkpoint of another model / library version; refusing to "
                "restart the %s silently" % (self._inner_cls.__name__, elements, tensors, eng.layout.total, len(eng.layout.slots), self._state_word))

    # ------------------------------------------------------------------ the inner optimizer
    def _fallback_step(self, rest):
        if not rest:
            return
        ids = tuple(id(p) for _, ps in rest for p in ps)
        if self._fallback is None or self._fallback_ids != ids:
            old = self._fallback
            groups = [dict(params=ps, **{k: g[k] for k in self._hyper}) for g, ps in rest]
            # (capturable=True reaches the inner optimizer of device tensors too: a composed module's step -- M_D.loss_and_grad
            # then step() -- can be captured into a graph like a fused model's.  Its fresh state then keeps the step counts on
            # the device.  A "fallback" state saved by a plain optimizer still loads: torch's load_state_dict takes the saved
            # groups, capturable=False among them, so such a state steps eagerly as it did and cannot be captured)
            flags = {}
            if self.defaults.get("capturable") and all(p.is_cuda for _, ps in rest for p in ps):
                flags["capturable"] = True
            self._fallback = self._inner_cls(groups, foreach=self.defaults["foreach"], **flags)
            self._fallback._mfm_inner = True        # (steps on behalf of this class: not a foreign optimizer)
            self._fallback_ids = ids
            self._inner_rebuilt(rest, old)
            if self._pending_fallback is not None:
                self._fallback.load_state_dict(self._pending_fallback)
                self._pending_fallback = None
        self._inner_stepping(ids)
        for fg, (g, _) in zip(self._fallback.param_groups, rest):
            for k in self._hyper:
                fg[k] = g[k]                        # schedulers act on OUR groups
        self._fallback.step()

    def _inner_stepping(self, ids):
        pass

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """torch's dict plus, under "fused", the flat state of every fused model (in the order the models appear in the
        parameter groups; the subclass's `_snapshot` says what an entry holds) and, under "fallback", the inner optimizer's"""
        sd = super().state_dict()
        fused = []
        for m, _ in self._fused_models():
            entry = self._snapshot(m, self._fused.get(m))
            if entry is not None:
                fused.append(entry)
        if self._pending_fused:          # loaded, not stepped yet: what was loaded is still the state
            fused += [dict(f) for f in self._pending_fused]
        sd["fused"] = fused
        if self._fallback is not None:
            sd["fallback"] = self._fallback.state_dict()
        return sd

    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        fused = sd.pop("fused", None)
        fb = sd.pop("fallback", None)
        super().load_state_dict(sd)
        self._fused.clear()
        self._pending_fused = [self._loaded_entry(f) for f in fused] if fused else None
        self._pending_fallback = fb

    # ------------------------------------------------------------------ Optimizer interface
    def step(self, closure=None):
        """Not wrapped by torch's `profile_hook_step` (`step.hooked` below): that wrapper opens a record_function scope around
        every step, ~10 us of host time against a 150 us device step the unchanged loop has to keep fed.  Step pre / post hooks
        registered on this optimizer or globally are still honoured."""
        if self._capture_refusal and _flat.capturing():
            raise _lib.MfmError(self._capture_refusal)
        hooks = self._optimizer_step_pre_hooks or self._optimizer_step_post_hooks or len(_GLOBAL_PRE) > 1 or _GLOBAL_POST
        if hooks:
            for h in list(_GLOBAL_PRE.values()) + list(self._optimizer_step_pre_hooks.values()):
                if h is not _foreign_step_hook:
                    h(self, (closure,) if closure is not None else (), {})
        prev = torch.is_grad_enabled()
        torch._C._set_grad_enabled(False)
        try:
            loss = self._step(closure)
        finally:
            torch._C._set_grad_enabled(prev)
        if hooks:
            for h in list(self._optimizer_step_post_hooks.values()) + list(_GLOBAL_POST.values()):
                h(self, (closure,) if closure is not None else (), {})
        return loss
    step.hooked = True

    def _step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        done, ndone = set(), 0
        for m, gidx in self._fused_models():
            if m._plist[0].is_cuda and self._fused_step(m, gidx):
                done.add(id(m))
                ndone += len(m._plist)
        if ndone == sum(len(g["params"]) for g in self.param_groups):
            return loss                               # (the reference's case: one model, nothing left)
        rest = []
        for group in self.param_groups:
            left = [p for p in group["params"] if id(_owner(p)) not in done] if done else list(group["params"])
            if left:
                rest.append((group, left))
        self._fallback_step(rest)
        return loss

    def zero_grad(self, set_to_none=True):
        cleared, nh = set(), 0
        for m, _ in self._fused_models():
            if getattr(m, "_grad_flat", None) is not None and m._grad_views_attached():
                m._zero_flat_grads(set_to_none)
                cleared.add(id(m))
                nh += len(m._plist)
        if nh == sum(len(g["params"]) for g in self.param_groups):
            return
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None or (cleared and id(_owner(p)) in cleared):
                    continue
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.zero_()


class Adam(_FlatOptimizer):
    """torch.optim.Adam (same signature, validation and arithmetic: weight decay, decoupled decay, AMSGrad, maximize, several
    parameter groups) whose fused models are updated by ONE launch per step.

    A fused model (`MFM_KL_EF`, `MFM_KL`, `MFM`) takes the flat path when the optimizer's parameter groups together hold all of
    its parameters.  A model that sits in one group with `weight_decay == 0`, `amsgrad` and `maximize` off -- the reference's
    call -- is stepped by `mfm_adam_flat_guarded` (`mfm_adam_flat_spans_guarded` when some tensors have no gradient,
    `mfm_adam_flat_dev` with `capturable=True`).  Any option, or a model spread over several groups, goes to
    `mfm_adam_ext_flat_spans_guarded`: each tensor is a span of the launch with its group's hyper-parameters and its own step
    count (adjacent tensors with equal values merge, so one group is one span).  Either way the model keeps its in-launch
    hand-overs.  A tensor without a gradient is skipped with all its state, its step count and its decoupled decay, as torch
    skips a parameter whose `.grad` is None.  Everything else -- other modules, a model only partly in the groups, frozen or
    hooked parameters, `fast_grads = False` -- goes through an inner torch.optim.Adam built with the same per-group options;
    moments, `max_exp_avg_sq` and step counts move between the two.

    The AMSGrad maximum is a third flat buffer per model (`_fused[m]["vmax"]`), allocated zero-filled on first need.
    `capturable=True` keeps the plain update only: an option or a second group per model is refused at construction."""

    _inner_cls = torch.optim.Adam
    _hyper = ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "decoupled_weight_decay")
    _state_word = "moments"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        # torch.optim.Adam's checks, in its order and with its messages
        if isinstance(lr, torch.Tensor):
            if foreach and not capturable:
                raise ValueError("lr as a Tensor is not supported for capturable=False and foreach=True")
            if lr.numel() != 1:
                raise ValueError("Tensor lr must be 1-element")
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
        if not ((isinstance(betas[0], float) and isinstance(betas[1], float))
                or (isinstance(betas[0], torch.Tensor) and isinstance(betas[1], torch.Tensor))):
            raise ValueError("betas must be either both floats or both Tensors")
        for k in (0, 1):
            if isinstance(betas[k], torch.Tensor):
                if not capturable and foreach:
                    raise ValueError(f"betas[{k}] as a Tensor is not supported for capturable=False and foreach=True")
                if betas[k].numel() != 1:
                    raise ValueError(f"Tensor betas[{k}] must be 1-element")
        betas = tuple(b.item() if isinstance(b, torch.Tensor) else b for b in betas)
        name = "factorized_amd.optim.%s" % type(self).__name__
        if differentiable:
            raise ValueError(name + ": differentiable=True is not built (the flat update is not part of the autograd graph); "
                             "use torch.optim." + type(self).__name__)
        if fused:
            raise ValueError(name + ": fused=True is torch's own fused kernel; this class fuses on its own (leave fused unset)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=False, fused=None,
                        decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)
        # capturable=True (torch.optim.Adam's flag): step count and learning rate of the fused update live in device memory
        # (mfm_adam_flat_dev), so a whole training step can be captured into a hipGraph and replayed (train.GraphedModuleStep)
        self._capturable = bool(capturable)
        models = self._init_flat()
        if self._capturable:
            if any(self._has_option(g) for g in self.param_groups) or any(not self._one_group(gidx) for _, gidx in models):
                raise ValueError(name + "(capturable=True): weight_decay, amsgrad, maximize and a model spread over several "
                                 "parameter groups are not built for the capturable update (one device-side step counter and "
                                 "learning rate per model); leave capturable off for them")

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:          # (a state saved before these options existed)
            for k in ("weight_decay", "amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused",
                      "decoupled_weight_decay"):
                group.setdefault(k, self.defaults[k])

    # ------------------------------------------------------------------ per-model state
    @staticmethod
    def _has_option(group):
        """an option the plain flat update does not compute (decay style alone changes nothing while weight_decay is 0)"""
        return group["weight_decay"] != 0 or bool(group["amsgrad"]) or bool(group["maximize"])

    @staticmethod
    def _one_group(gidx):
        return bool((gidx == gidx[0]).all())

    @staticmethod
    def _stale(st, eng):
        return st["m"].numel() != eng.layout.total or st["m"].device != eng.params.device

    @staticmethod
    def _new_state(eng):
        """flat moments and per-tensor step counts; vmax: the AMSGrad maximum of v, allocated on first need (_vmax)"""
        return dict(m=torch.zeros_like(eng.params), v=torch.zeros_like(eng.params), vmax=None,
                    steps=np.zeros(len(eng.layout.slots), dtype=np.int64))

    def _restore(self, st, saved, eng):
        vmax = saved.get("vmax")
        self._require_fit(saved["m"].numel(), len(saved["steps"]), eng, vmax is None or vmax.numel() == eng.layout.total)
        st["m"].copy_(saved["m"]); st["v"].copy_(saved["v"])
        st["steps"][:] = np.asarray(saved["steps"], dtype=np.int64)
        if vmax is not None:
            st["vmax"] = vmax.to(eng.params.device, copy=True)

    @staticmethod
    def _vmax(st):
        if st["vmax"] is None:
            st["vmax"] = torch.zeros_like(st["v"])
        return st["vmax"]

    def _device_scalars(self, st, eng, lr):
        """capturable mode: the step counter and the learning rate as device words of this model's state"""
        dev = eng.params.device
        if "step_dev" not in st:
            st["step_dev"] = torch.full((1,), int(st["steps"][0]), dtype=torch.int32, device=dev)
            st["lr_dev"] = torch.zeros(1, dtype=torch.float32, device=dev)
            st["lr_host"] = None
        if torch.is_tensor(lr):
            if lr.is_cuda and lr.dtype == torch.float32:
                return st["step_dev"], lr                     # the caller's own device scalar (GraphedModuleStep.set_lr)
            lr = float(lr)
        if st["lr_host"] != lr:
            if _flat.capturing():
                raise _lib.MfmError("factorized_amd.optim.Adam(capturable=True): the learning rate changed inside a stream "
                                    "capture; pass lr as a float32 device tensor or change it between replays")
            st["lr_dev"].fill_(lr)
            st["lr_host"] = lr
        return st["step_dev"], st["lr_dev"]

    def _migrate_back(self, m, st, eng):
        """a model returns to the flat path after steps through the stock optimizer (a parameter was frozen and is trainable
        again): moments and step counts the stock optimizer holds for its tensors come back into the flat state"""
        fb = self._fallback
        if fb is None:
            return
        for i, p in enumerate(m._plist):
            s = fb.state.get(p)
            if not s:
                continue
            o, n, shp = eng.layout.slots[i]
            st["m"][o:o + n].view(shp).copy_(s["exp_avg"])
            st["v"][o:o + n].view(shp).copy_(s["exp_avg_sq"])
            if "max_exp_avg_sq" in s:
                self._vmax(st)[o:o + n].view(shp).copy_(s["max_exp_avg_sq"])
            st["steps"][i] = int(float(s["step"]))
            del fb.state[p]
        if "step_dev" in st:
            st["step_dev"].fill_(int(st["steps"].max()))

    # ------------------------------------------------------------------ the update
    def _fused_step(self, m, gidx):
        eng = m.engine
        group = self.param_groups[gidx[0]]
        plain = self._one_group(gidx) and not self._has_option(group)
        if self._capturable and not plain:
            raise _lib.MfmError("factorized_amd.optim.Adam(capturable=True): weight_decay, amsgrad, maximize and a model spread "
                                "over several parameter groups are not built for the capturable update")
        gflat = self._flat_grads(m, eng)
        if gflat is None:
            return False
        st = self._state_for(m, eng)
        if self._fallback is not None and self._fallback.state:
            self._migrate_back(m, st, eng)
        if not plain:
            return self._ext_step(m, gidx, st, gflat)
        lr, (b1, b2), eps = group["lr"], group["betas"], group["eps"]
        if torch.is_tensor(lr) and not self._capturable:
            lr = float(lr)
        present = m._grad_present
        L = _lib.lib()
        stream, guard = _stream_and_guard(eng, gflat)
        head = (_ptr(eng.params), _ptr(gflat), _ptr(st["m"]), _ptr(st["v"]))
        steps = st["steps"]
        if self._capturable:
            if not (present.all() and (steps == steps[0]).all()):
                raise _lib.MfmError("factorized_amd.optim.Adam(capturable=True): every tensor needs a gradient in every step (one "
                                    "device-side step counter); staged losses train through the eager optimizer")
            step_dev, lr_dev = self._device_scalars(st, eng, group["lr"])
            _lib.check(L.mfm_adam_flat_dev(*head, eng.layout.total, _ptr(step_dev), _ptr(lr_dev), b1, b2, eps, 1.0, guard, stream),
                       "mfm_adam_flat_dev")
            steps += 1           # (host mirror: exact in eager use, a lower bound under graph replay -- see _snapshot())
            return True
        if present.all() and (steps == steps[0]).all():
            steps += 1
            _lib.check(L.mfm_adam_flat_guarded(*head, eng.layout.total, int(steps[0]), lr, b1, b2, eps, 1.0, guard, stream),
                       "mfm_adam_flat_guarded")
            return True
        # some tensors have no gradient (stage losses, unused layers): contiguous runs of present tensors with equal
        # step counts become spans
        steps[present] += 1
        spans = _flat.merge_spans(st["order"], st["extents"], present, [(s,) for s in steps.tolist()])
        _flat.launch_tables(L.mfm_adam_flat_spans_guarded, "mfm_adam_flat_spans_guarded", head,
                            _flat.span_tables(spans, _lib.AdamSpan, _lib.MFM_ADAM_MAX_SPANS, ("step",)),
                            (lr, b1, b2, eps, 1.0, guard, stream))
        return True

    _EXT_FIELDS = ("lr", "beta1", "beta2", "eps", "weight_decay", "flags", "step")

    def _ext_step(self, m, gidx, st, gflat):
        """an option (weight decay, AMSGrad, maximize) or several groups: every tensor with a gradient is a span of ONE launch of
        mfm_adam_ext_flat_spans_guarded with its group's hyper-parameters and its own step count; adjacent tensors whose values
        and step counts agree merge (one group, every tensor present: one span)"""
        eng = m.engine
        hyper = []
        for g in self.param_groups:
            fl = ((_lib.MFM_ADAMX_MAXIMIZE if g["maximize"] else 0) | (_lib.MFM_ADAMX_AMSGRAD if g["amsgrad"] else 0)
                  | (_lib.MFM_ADAMX_DECOUPLED if g["decoupled_weight_decay"] else 0))
            hyper.append((float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), fl))
        # (layers no forward uses carry a zero gradient on the flat path; torch's .grad is None there: no decay, no step count)
        present, steps = m._grad_present & ~m._group_masks()["unreached"], st["steps"]
        order, extents = st["order"], st["extents"]
        if "runs" not in st or st["runs"][0] is not gidx:
            # the runs (begin, end, group) of adjacent tensors of one group
            st["runs"] = (gidx, order, extents, _flat.merge_spans(order, extents, np.ones(len(order), dtype=bool), gidx.tolist()))
        if present.all() and (steps == steps[0]).all():
            steps += 1
            s_ = int(steps[0])
            spans = [(b, e, hyper[gi] + (s_,)) for b, e, gi in st["runs"][3]]
        else:
            # no gradient: moments, vmax, step count and decoupled decay all stay (torch skips it)
            steps[present] += 1
            spans = _flat.merge_spans(order, extents, present, [hyper[gi] + (s,) for gi, s in zip(gidx.tolist(), steps.tolist())])
        if not spans:
            return True                  # no tensor has a gradient: torch's step does nothing either
        amsgrad = any(key[5] & _lib.MFM_ADAMX_AMSGRAD for _, _, key in spans)
        stream, guard = _stream_and_guard(eng, gflat)       # (a NaN guard leaves vmax alone too)
        vmax = _ptr(self._vmax(st)) if amsgrad else C.c_void_p(None)
        _flat.launch_tables(_lib.lib().mfm_adam_ext_flat_spans_guarded, "mfm_adam_ext_flat_spans_guarded",
                            (_ptr(eng.params), _ptr(gflat), _ptr(st["m"]), _ptr(st["v"]), vmax),
                            _flat.span_tables(spans, _lib.AdamExtSpan, _lib.MFM_ADAMX_MAX_SPANS, self._EXT_FIELDS),
                            (1.0, guard, stream))
        return True

    def _inner_rebuilt(self, rest, old):
        """parameters of a fused model that now go through the stock optimizer (a parameter was frozen / got a hook after
        fast-path steps): their moments and step counts move along -- Adam must not restart"""
        for g, ps in rest:
            for p in ps:
                m = _owner(p)
                st = self._fused.get(m) if m is not None else None
                if st is None or p in self._fallback.state:
                    continue
                i = next((k for k, q in enumerate(m._plist) if q is p), None)
                if i is None:
                    continue
                o, n, shp = m.engine.layout.slots[i]
                steps = int(st["step_dev"].item()) if "step_dev" in st else int(st["steps"][i])
                if steps == 0:
                    continue
                self._fallback.state[p] = dict(step=torch.tensor(float(steps)), exp_avg=st["m"][o:o + n].view(shp).clone(),
                                               exp_avg_sq=st["v"][o:o + n].view(shp).clone())
                if g["amsgrad"]:
                    self._fallback.state[p]["max_exp_avg_sq"] = self._vmax(st)[o:o + n].view(shp).clone()
        # (the flat state stays: when the model returns to the flat path, _migrate_back brings the moments home instead of
        #  restarting them from zero)

    def reset_state(self):
        """moments and step counters of every fused model back to zero, in place (a captured graph keeps pointing at them)"""
        for st in self._fused.values():
            st["m"].zero_(); st["v"].zero_(); st["steps"][:] = 0
            if st["vmax"] is not None:
                st["vmax"].zero_()
            if "step_dev" in st:
                st["step_dev"].zero_()

    # ------------------------------------------------------------------ checkpoints
    def _snapshot(self, m, st):
        """a "fused" entry: first / second moments and per-tensor step counts (capturable mode: the device counter)"""
        if st is None:
            return None
        steps = st["steps"].copy()
        if "step_dev" in st:
            steps[:] = int(st["step_dev"].item())
        entry = dict(m=st["m"].detach().clone(), v=st["v"].detach().clone(), steps=steps.tolist())
        if st["vmax"] is not None:       # (AMSGrad only: a state without it keeps the keys it always had)
            entry["vmax"] = st["vmax"].detach().clone()
        return entry

    @staticmethod
    def _loaded_entry(f):
        return dict(f, steps=list(f["steps"]))


class AdamW(Adam):
    """torch.optim.AdamW: `Adam` with torch's AdamW defaults and decoupled weight decay forced on (as torch.optim.AdamW derives
    from torch.optim.Adam)"""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize,
                         capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=True)


class SGD(_FlatOptimizer):
    """torch.optim.SGD with momentum (same signature, validation and arithmetic) whose fused models are updated by ONE launch of
    `mfm_sgd_flat_spans_guarded` per step: the reference's other optimizer line (mfm_mosi.py:404, commented out under the Adam
    line in every driver).

    A fused model (`MFM_KL_EF`, `MFM_KL`, `MFM`) takes the flat path when the optimizer's parameter groups together hold all of
    its parameters -- one group or several: each tensor becomes a span of the launch with its group's hyper-parameters
    (adjacent tensors with equal values merge).  Such a model keeps its in-launch hand-overs (the update honours the gradient
    guard).  A tensor without a gradient is skipped, its momentum buffer included, as torch skips a parameter whose `.grad` is
    None; `zero_grad(set_to_none=False)` keeps zero gradients in place, so a tensor that once had a gradient keeps moving on its
    momentum (the reference's PyTorch 0.4).  Everything else -- other modules, a model only partly in the groups, frozen or
    hooked parameters, `fast_grads = False` -- goes through an inner torch.optim.SGD; momentum buffers move between the two.

    Momentum buffers are kept per model as ONE flat buffer plus a per-tensor "buffer exists" flag (torch's
    `state[p]["momentum_buffer"] is not None`); the slot of a tensor whose flag is False always holds zeros (every place that
    clears a flag clears the slot).  A step the gradient guard skipped writes nothing, yet the host has already marked the
    buffers of that step's first-step tensors as existing.  With dampening 0 that is exact: the slot still holds zeros and
    `momentum * 0 + d` is the first step's `d`.  With dampening != 0 it is not, so such a step also copies the guard word aside,
    and the next step (or state_dict()) reads it -- one synchronisation, once per first step -- and, if the step was skipped,
    marks those buffers as not existing again.

    Which side holds a model's live buffers is tracked per model: a model that steps through the inner optimizer (from its
    first step on, or after flat steps) is "away", and its next flat step takes the inner optimizer's buffers back."""

    _inner_cls = torch.optim.SGD
    _hyper = ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize")
    _state_word = "momentum"
    _capture_refusal = ("factorized_amd.optim.SGD.step() inside a stream capture: the SGD update is eager only "
                        "(hipGraph capture of a training step: train.GraphedModuleStep with optim.Adam(capturable=True))")

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None):
        # torch.optim.SGD's checks, in its order and with its messages
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if differentiable:
            raise ValueError("factorized_amd.optim.SGD: differentiable=True is not built (the flat update is not part of the "
                             "autograd graph); use torch.optim.SGD")
        if fused:
            raise ValueError("factorized_amd.optim.SGD: fused=True is torch's own fused kernel; this class fuses on its own "
                             "(leave fused unset)")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=foreach, differentiable=False, fused=None)
        super().__init__(params, defaults)
        # fused models whose live momentum buffers are in the inner optimizer (they stepped through it since their last flat step)
        self._away = weakref.WeakSet()
        self._init_flat()

    # ------------------------------------------------------------------ per-model state
    @staticmethod
    def _stale(st, eng):
        return st["total"] != eng.layout.total or (st["buf"] is not None and st["buf"].device != eng.params.device)

    @staticmethod
    def _new_state(eng):
        """the flat momentum buffer (None before any momentum step), the per-tensor "buffer exists" flags, the first-step
        bookkeeping of the class doc (pending, gseen) and the span tables of earlier steps"""
        return dict(total=eng.layout.total, buf=None, have=np.zeros(len(eng.layout.slots), dtype=bool), pending=None, gseen=None,
                    spans={})

    def _restore(self, st, saved, eng):
        self._require_fit(saved["total"], len(saved["have"]), eng)
        st["have"][:] = np.asarray(saved["have"], dtype=bool)
        if saved["buf"] is not None:
            st["buf"] = saved["buf"].to(eng.params.device, copy=True)
            for i in np.flatnonzero(~st["have"]):
                o, k, _ = eng.layout.slots[i]
                st["buf"][o:o + k].zero_()       # (no buffer: a zero slot, whatever the checkpoint held there)

    @staticmethod
    def _resolve_pending(st):
        """a first step with dampening != 0 that the guard may have skipped: read the guard word it saw (see the class doc)"""
        if st["pending"] is not None:
            if not float(st["gseen"].item()) == 0.0:
                st["have"][st["pending"]] = False
            st["pending"] = None

    def _buf(self, st, like):
        if st["buf"] is None:
            st["buf"] = torch.zeros_like(like)
        return st["buf"]

    def _migrate_back(self, m, st, eng):
        """the model returns to the flat path after steps through the inner optimizer: its momentum buffers (the live ones) come
        back into the flat state"""
        fb = self._fallback
        for i, p in enumerate(m._plist):
            s = fb.state.get(p) if fb is not None else None
            b = s.get("momentum_buffer") if s else None
            o, n, shp = eng.layout.slots[i]
            if b is not None:
                self._buf(st, eng.params)[o:o + n].view(shp).copy_(b)
            elif st["buf"] is not None:
                st["buf"][o:o + n].zero_()
            st["have"][i] = b is not None
            if s is not None:
                del fb.state[p]
        st["spans"].clear()

    def _migrate_out(self, m, st):
        """the model steps through the inner optimizer (a parameter was frozen / got a hook): its momentum buffers move there --
        on every such switch, so that freeze -> unfreeze -> freeze keeps the momentum"""
        self._resolve_pending(st)
        fb = self._fallback
        for i, p in enumerate(m._plist):
            if st["have"][i]:
                o, n, shp = m.engine.layout.slots[i]
                fb.state[p] = dict(momentum_buffer=st["buf"][o:o + n].view(shp).clone())
            else:
                fb.state.pop(p, None)

    # ------------------------------------------------------------------ the update
    _FIELDS = ("lr", "weight_decay", "momentum", "dampening", "flags")

    def _spans_of(self, st, present, gidx):
        """ctypes span tables for this step (cached per pattern of present tensors, existing buffers and hyper-parameters)"""
        hyper = tuple((float(g["lr"]), float(g["weight_decay"]), float(g["momentum"]), float(g["dampening"]),
                       (_lib.MFM_SGD_NESTEROV if g["nesterov"] else 0) | (_lib.MFM_SGD_MAXIMIZE if g["maximize"] else 0))
                      for g in self.param_groups)
        have = st["have"]
        key = (present.tobytes(), have.tobytes(), hyper)
        hit = st["spans"].get(key)
        if hit is not None:
            return hit
        keys, first, first_damp = [None] * len(have), [], []
        for i in np.flatnonzero(present):
            lr, wd, mom, damp, fl = hyper[gidx[i]]
            if mom != 0.0 and not have[i]:
                fl |= _lib.MFM_SGD_FIRST
                first.append(i)
                if damp != 0.0:
                    first_damp.append(i)
            keys[i] = (lr, wd, mom, damp, fl)
        spans = _flat.merge_spans(st["order"], st["extents"], present, keys)
        tables = _flat.span_tables(spans, _lib.SgdSpan, _lib.MFM_SGD_MAX_SPANS, self._FIELDS)
        momentum = any(h[2] != 0.0 for _, _, h in spans)
        hit = (tables, np.array(first, dtype=np.int64), np.array(first_damp, dtype=np.int64), momentum)
        if len(st["spans"]) > 32:
            st["spans"].clear()
        st["spans"][key] = hit
        return hit

    def _fused_step(self, m, gidx):
        eng = m.engine
        gflat = self._flat_grads(m, eng)
        if gflat is None:
            return False
        st = self._state_for(m, eng)
        if m in self._away:
            self._migrate_back(m, st, eng)
            self._away.discard(m)
        self._resolve_pending(st)
        tables, first, first_damp, momentum = self._spans_of(st, m._grad_present, gidx)
        if not tables:
            return True                      # no tensor has a gradient: torch's step does nothing either
        stream, guard = _stream_and_guard(eng, gflat)
        buf = _ptr(self._buf(st, eng.params)) if momentum else C.c_void_p(None)
        _flat.launch_tables(_lib.lib().mfm_sgd_flat_spans_guarded, "mfm_sgd_flat_spans_guarded",
                            (_ptr(eng.params), _ptr(gflat), buf), tables, (1.0, guard, stream))
        if len(first):
            st["have"][first] = True
            if len(first_damp):
                if st["gseen"] is None:
                    st["gseen"] = torch.zeros(1, dtype=torch.float32, device=eng.params.device)
                g = eng.layout.guard
                st["gseen"].copy_(gflat[g:g + 1])
                st["pending"] = first_damp
        return True

    def _inner_rebuilt(self, rest, old):
        if old is not None:                     # buffers of tensors that stay with the inner optimizer stay too
            idset = set(self._fallback_ids)
            for p, s in old.state.items():
                if id(p) in idset:
                    self._fallback.state[p] = s

    def _inner_stepping(self, ids):
        idset = set(ids)
        for m, _ in self._fused_models():
            if m in self._away or id(m._plist[0]) not in idset or not m._plist[0].is_cuda:
                continue
            # a fused model starts stepping through the inner optimizer: its flat buffers (if it has any, or a checkpoint's
            # waiting for it) go there, and its next flat step takes them back
            st = self._fused.get(m)
            if st is None and self._pending_fused:
                st = self._state_for(m, m.engine)
            if st is not None:
                self._migrate_out(m, st)
            self._away.add(m)

    # ------------------------------------------------------------------ checkpoints
    def _snapshot(self, m, st):
        """a "fused" entry: the model's flat momentum buffer (None before any momentum step) and the per-tensor "buffer exists"
        flags"""
        away = m in self._away
        if st is None and not away:
            return None
        if not away:
            self._resolve_pending(st)
            buf = st["buf"].detach().clone() if st["buf"] is not None else None
            have = st["have"].tolist()
        else:                            # stepping through the inner optimizer: its buffers are the live ones
            eng = m.engine
            buf, have = torch.zeros_like(eng.params), []
            for i, p in enumerate(m._plist):
                b = self._fallback.state.get(p, {}).get("momentum_buffer")
                if b is not None:
                    o, n, shp = eng.layout.slots[i]
                    buf[o:o + n].view(shp).copy_(b)
                have.append(b is not None)
        return dict(total=m.engine.layout.total, buf=buf, have=have)

    @staticmethod
    def _loaded_entry(f):
        return dict(total=int(f["total"]), buf=f["buf"], have=list(f["have"]))

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._away = weakref.WeakSet()      # (the loaded fused entries hold every model's live buffers)
        if self._fallback is not None and self._pending_fallback is not None:
            self._fallback.load_state_dict(self._pending_fallback)
            self._pending_fallback = None
