"""Keep the best model without leaving the device: what the reference's end-of-epoch lines do with a pickle on disk
(mfm_mosi.py:467-481, the same in mfm_you.py / mfm_moud.py / mfm_mmmo.py)

    if valid_loss <= best_valid:
        best_valid = valid_loss
        torch.save(model, 'res_mfm2/mfn_%d.pt' % rand)
    ...
    model = torch.load('res_mfm2/mfn_%d.pt' % rand)

becomes

    from factorized_amd.checkpoint import KeepBest
    best = KeepBest(model, mode="min", initial=None)     # initial: +inf / -inf by mode; the reference's 999999.0 may be passed
    ...
    took = best.update(valid_loss)     # python float, 0-d tensor (CPU or device), or a lazy LossExpr
    ...
    best.restore()                     # model <- best weights
    best.value, best.epoch, best.calls # host reads (synchronise)

The rule is the reference's `<=` (mode "max": `>=`): a tie takes the newer weights, a NaN metric never takes.  The metric is
compared in fp32 on both paths (a python float is rounded to fp32 first), so the two paths take the same decisions.  `epoch`
is the 0-based index of the `update` call that last took a snapshot (-1: none yet), `calls` the number of `update` calls.

Flat path.  When `model` is a fused model (`MFM_KL_EF`, `MFM_KL`, `MFM`, or the `.module` of a `swa_utils.AveragedModel`) on the
GPU whose parameters are the views of its engine's flat fp32 buffer, all trainable, `update` is ONE launch of
`mfm_keep_best_flat` (csrc/keep_best.hip) on the current stream over [offset of the first tensor, layout.guard) -- the range
`swa_utils` uses: the comparison, the conditional copy and the bookkeeping happen on the device.

  * No host synchronisation, and no allocation after the first call.  A 0-d fp32 tensor on the model's device goes in by
    pointer; a `LossExpr` is evaluated to such a tensor by the kernels that materialise its value anywhere else (that result
    comes from the caching allocator); a python float or a CPU tensor goes in as the launch's scalar argument.  A device tensor
    of another dtype is converted to fp32 on the device first.
  * Inside a stream capture only the device form is accepted: a host value would be baked into the graph and every replay
    would compare the same number, so `_lib.MfmError` is raised.  A replayed launch decides anew and keeps counting.
  * `update` returns a 0-d int32 view of the state's `taken` word: no launch, and `bool(took)` synchronises only if the caller
    asks.  It is a view of live state: the next `update` overwrites it.
  * The snapshot buffer and the state block with its ticket word are allocated on first use, outside a capture; pickling and
    `copy.deepcopy` drop the ticket (a copy draws its own).  Model and engine are re-validated on every call with the pointer
    checks of `_FusedEngineMixin._flat_ok`; the metric argument and the state block are `_flat.metric_arg` / `_flat.pack_words`.

`restore()` is one `copy_` of the range back into the live flat buffer.  After it the model is in the state
`model.load_state_dict(<the same values>)` leaves it in.  What was checked for that: `nn.Module.load_state_dict` on a fused model
is a per-tensor `param.copy_()` into the views of the flat buffer and nothing else (the model classes override neither it nor
`_load_from_state_dict`); the plans keep no image of the weights between calls (the bf16 weight images are rebuilt by the pack
launch of every forward, csrc/plan_forward.hip); and the bookkeeping `engine.load_weights` resets beyond the copy (`adam_m`,
`adam_v`, `step_count`, `group_steps`) belongs to `engine.train_step`'s own optimizer, which `load_state_dict` does not touch
either.  So the copy is all there is to do; the padding between tensors travels with the range and holds what it held at the
snapshot.  Gradients and optimizer moments are not touched: the reference saves the model only, so snapshotting the optimizer
is out of scope -- a run that goes on training after `restore()` keeps the moments it had.

Everything else -- CPU models, the composed models of mfm_extra.py, any other nn.Module, a fused model with a frozen parameter,
with buffers or off its flat buffer -- goes through plain torch: the metric is read to a python float, the rule applied on the
host, and the snapshot is a per-tensor clone of `state_dict()` refreshed with `torch._foreach_copy_`.  Semantics and attributes
are the same and the path is always correct.  The two paths may alternate on one instance: state and snapshot move with it
(that hand-over reads the state back, i.e. synchronises, once).

Inside a stream capture such a module takes a third form, so that `evaluate -> scheduler.step -> best.update` of the composed
classes that return a device loss (`M_B`, `M_D`) is one graph.  A torch-path `update` with a device metric on a module whose
tensors live on one GPU leaves the state block and per-tensor snapshot buffers beside the model (one small upload; make that
call outside the capture first, else `_lib.MfmError`).  The captured `update` applies the same fp32 rule with torch operations
on them -- the comparison, one conditional copy per tensor, the bookkeeping -- and returns the 0-d int32 `taken` word;
`last_path` is "tensors".  Replays move the block; `value`, `calls`, `epoch`, `taken`, `restore()` and `state_dict()` read it
back, and an `update` outside the capture goes on from it on the torch path and uploads the result again.

`state_dict()` / `load_state_dict()` carry the mode, `value`, `calls`, `epoch` and the snapshot under the model's own parameter
names, so a KeepBest survives a checkpoint of the run on either path.

Data parallel: ranks that pass the same metric (the all-reduced validation loss) take the same decision from the same rule,
so the replicas' snapshots stay in step without any communication; no collective is involved."""
import ctypes as C
from collections import OrderedDict

import torch

from . import _flat, _lib
from ._fused import _FusedEngineMixin

__all__ = ["KeepBest"]

_MODES = {"min": _lib.MFM_KEEP_MIN, "max": _lib.MFM_KEEP_MAX}
# MfmKeepBestState as int32 words; _STATE: the words the host form holds, in the order of (_value, _calls, _best_call, _taken)
_W_VALUE, _W_CALLS, _W_BEST_CALL, _W_TAKEN, _W_TICKET = 0, 1, 2, 3, 4
_STATE = ((_W_VALUE, "float32"), (_W_CALLS, "int32"), (_W_BEST_CALL, "int32"), (_W_TAKEN, "int32"))


def _fp32(v):
    """a python number as the fp32 value the kernel would compare (overflow -> inf, NaN stays)"""
    return C.c_float(float(v)).value


class KeepBest:
    """Remember the model's weights whenever the metric is at least as good as the best so far (see the module doc)."""

    def __init__(self, model, mode="min", initial=None):
        if mode not in _MODES:
            raise ValueError("KeepBest: mode must be 'min' or 'max', not %r" % (mode,))
        self.model = model
        self.mode = mode
        if initial is None:
            initial = float("inf") if mode == "min" else float("-inf")
        self.initial = _fp32(initial)
        self.last_path = None            # "flat" / "torch": the path of the latest update
        # host form of the state (authoritative while _on_device is False)
        self._value, self._calls, self._best_call, self._taken = self.initial, 0, -1, 0
        self._snap = None                # torch path: OrderedDict name -> clone, once a snapshot was taken
        # device form (authoritative while _on_device is True)
        self._on_device = False
        self._mfm_state = None           # int32[MFM_KEEP_STATE_WORDS] on the model's device
        self._mfm_ticket = None          # its ticket word (a view)
        self._mfm_taken = None           # its taken word (a 0-d view: what update returns)
        self._mfm_flat = None            # snapshot buffer with the engine's layout
        self._mfm_key = None             # (engine, layout) the buffers were last validated against
        # tensor form (any other module on one GPU, see the module doc): the state block again, the snapshot per tensor
        self._td_state = None            # int32[MFM_KEEP_STATE_WORDS] beside the model, in step with the host form after every
        self._td_snap = None             # torch-path update; name -> tensor, the buffers `_snap` names once a snapshot was taken
        self._td_fresh = False           # the block holds the host form's values
        self._td_live = False            # a captured update was recorded: replays move the block, host reads read it back

    # ------------------------------------------------------------------ copies
    def __getstate__(self):
        state = dict(self.__dict__)
        state["_mfm_ticket"] = None          # (never shared with a copy: each instance draws its own tickets)
        state["_mfm_taken"] = None
        state["_mfm_key"] = None             # (an engine does not travel; re-validated on the next call)
        if self._td_live:                    # (a copy has no graph that moves its block: it goes on from the values read back)
            host = dict(zip(("_value", "_calls", "_best_call", "_taken"), _flat.unpack_words(self._td_state.cpu(), _STATE)))
            state.update(host, _snap=self._td_snap if host["_best_call"] >= 0 else None)
        state.update(_td_state=None, _td_snap=None, _td_fresh=False, _td_live=False)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)

    # ------------------------------------------------------------------ which path
    def _flat_engine(self):
        """the engine of a model that can take the flat path, else None (cheap: pointer checks, one walk over requires_grad)"""
        m = self.model
        if not isinstance(m, _FusedEngineMixin) or not m._plist or not m._plist[0].is_cuda or not m._flat_ok():
            return None
        for p in m._plist:
            if not p.requires_grad:
                return None
        eng = m._engine
        key = self._mfm_key
        if key is None or key[0] is not eng or key[1] is not eng.layout:
            # (once per engine: a module with buffers has a state_dict the flat range does not cover)
            if _flat.has_buffers(m):
                return None
            self._mfm_key = (eng, eng.layout)
        return eng

    # ------------------------------------------------------------------ hand-over between the two forms of the state
    def _to_device(self, eng):
        """state and snapshot into device memory beside `eng` (first flat call, or the first one after torch-path calls)"""
        dev = eng.params.device
        fresh = (self._mfm_state is None or self._mfm_state.device != dev or self._mfm_flat is None
                 or self._mfm_flat.device != dev or self._mfm_flat.numel() != eng.layout.total or self._mfm_ticket is None)
        if (fresh or not self._on_device) and _flat.capturing():
            raise _lib.MfmError("KeepBest.update: the snapshot buffer and the state block are set up on the first call on the "
                                "flat path; make that call outside the stream capture")
        if self._on_device and not fresh:
            return
        if self._on_device:                      # the device changed, or a copy dropped the ticket: carry the state over
            self._read_back()
        if self._mfm_flat is None or self._mfm_flat.device != dev or self._mfm_flat.numel() != eng.layout.total:
            self._mfm_flat = torch.zeros_like(eng.params)
        if self._snap is not None:
            views = eng.layout.views(self._mfm_flat)
            names = list(views)
            if list(self._snap) != names:
                raise _lib.MfmError("KeepBest: the snapshot's tensors do not match the model's parameters")
            torch._foreach_copy_([views[n] for n in names], [self._snap[n].to(dev) for n in names])
            self._snap = None
        values = (self._value, self._calls, self._best_call, self._taken)
        self._mfm_state = _flat.pack_words(_lib.MFM_KEEP_STATE_WORDS, [(w, kind, v) for (w, kind), v in zip(_STATE, values)]).to(dev)
        self._mfm_ticket = self._mfm_state[_W_TICKET:_W_TICKET + 1]
        self._mfm_taken = self._mfm_state[_W_TAKEN]
        self._on_device = True

    def _read_back(self):
        """the device state into the host fields (synchronises); the device form stays authoritative"""
        self._value, self._calls, self._best_call, self._taken = _flat.unpack_words(self._mfm_state.cpu(), _STATE)

    # ------------------------------------------------------------------ the tensor form: a captured update of any GPU module
    def _td_read_back(self):
        """what the replays of a captured update left in the block into the host form (synchronises); the replays may go on"""
        if not self._td_live:
            return
        self._value, self._calls, self._best_call, self._taken = _flat.unpack_words(self._td_state.cpu(), _STATE)
        self._snap = self._td_snap if self._best_call >= 0 else None

    def _td_device(self):
        """the one GPU every tensor of the model's state_dict lives on, else None"""
        devs = {t.device for t in self.model.state_dict().values()}
        dev = next(iter(devs)) if len(devs) == 1 else None
        return dev if dev is not None and dev.type == "cuda" else None

    def _td_upload(self, dev):
        """the host form into the block beside the model (outside a capture, behind a torch-path update)"""
        sd = self.model.state_dict()
        snap = self._snap if self._snap is not None else self._td_snap
        if (snap is None or list(snap) != list(sd)
                or any(a.shape != b.shape or a.device != b.device or a.dtype != b.dtype for a, b in zip(snap.values(), sd.values()))):
            snap = OrderedDict((k, t.detach().clone()) for k, t in sd.items())      # (buffers alone: no snapshot was taken yet)
        self._td_snap = snap
        values = (self._value, self._calls, self._best_call, self._taken)
        host = _flat.pack_words(_lib.MFM_KEEP_STATE_WORDS, [(w, kind, v) for (w, kind), v in zip(_STATE, values)])
        if self._td_state is None or self._td_state.device != dev:
            self._td_state = host.to(dev)
        else:
            self._td_state.copy_(host)
        self._td_fresh = True

    def _update_tensors(self, metric):
        """update() inside a stream capture for a module off the flat path: the rule, the conditional copies and the bookkeeping
        as torch operations on the block and the snapshot buffers a torch-path update left beside the model"""
        sd = self.model.state_dict()
        snap = self._td_snap
        if (not self._td_fresh or self._td_state is None or snap is None or list(snap) != list(sd)
                or any(a.shape != b.shape or a.device != b.device or a.dtype != b.dtype for a, b in zip(snap.values(), sd.values()))):
            raise _lib.MfmError("KeepBest.update: inside a stream capture a model off the flat path needs the state block and the "
                                "snapshot buffers that an update with a device metric sets up; make that call outside the "
                                "stream capture first")
        st = self._td_state
        with torch.no_grad():
            v = metric.detach().to(device=st.device, dtype=torch.float32).reshape(())
            best = st[_W_VALUE:_W_VALUE + 1].view(torch.float32)[0]             # (0-d views of the block's words)
            calls, best_call, taken = st[_W_CALLS], st[_W_BEST_CALL], st[_W_TAKEN]
            take = v <= best if self.mode == "min" else v >= best          # (False for a NaN)
            for dst, src in zip(snap.values(), sd.values()):
                dst.copy_(torch.where(take, src.detach(), dst))
            best.copy_(torch.where(take, v, best))
            best_call.copy_(torch.where(take, calls, best_call))
            taken.copy_(take.to(torch.int32))
            calls.add_(1)
        self._td_live = True
        self.last_path = "tensors"
        return st[_W_TAKEN]

    def _to_host(self):
        """state and snapshot into the torch-path form (synchronises; the first torch-path call after flat ones)"""
        if not self._on_device:
            return
        self._read_back()
        self._on_device = False
        self._snap = self._flat_snapshot() if self._best_call >= 0 else None

    def _flat_snapshot(self):
        """the flat snapshot as clones under the model's parameter names"""
        names = self.model._param_names
        key = self._mfm_key
        layout = key[1] if key is not None else None
        if layout is None or list(layout.shapes) != names or layout.total != self._mfm_flat.numel():
            from . import engine as E
            layout = E.FlatLayout(OrderedDict((n, tuple(p.shape)) for n, p in zip(names, self.model._plist)),
                                  self.model._engine_variant)
        return OrderedDict((n, v.clone()) for n, v in layout.views(self._mfm_flat).items())

    # ------------------------------------------------------------------ update
    def update(self, metric):
        """Compare `metric` with the best so far and snapshot the model if it is at least as good.  Returns 0-d int32: 1 if this
        call took a snapshot (flat path: a view of device state, no synchronisation until it is read)."""
        eng = self._flat_engine()
        if eng is None:
            if _flat.capturing() and isinstance(metric, torch.Tensor) and metric.is_cuda and metric.numel() == 1:
                return self._update_tensors(metric)
            return self._update_torch(metric)
        self._td_read_back()
        self._td_fresh = self._td_live = False
        dev = eng.params.device
        keep, host = _flat.metric_arg(metric, dev, "KeepBest.update", "the model's device")      # (keep: alive over the launch)
        ptr, scalar = (keep.data_ptr(), 0.0) if keep is not None else (None, _fp32(host))
        self._to_device(eng)
        _lib.check(_lib.lib().mfm_keep_best_flat(_flat.ptr(self._mfm_flat), _flat.ptr(eng.params), eng.layout.begin, eng.layout.guard,
                                                 _MODES[self.mode], C.c_void_p(ptr), scalar, _flat.ptr(self._mfm_state),
                                                 _flat.stream_ptr(dev)), "mfm_keep_best_flat")
        self.last_path = "flat"
        return self._mfm_taken

    def _update_torch(self, metric):
        self._to_host()
        self._td_read_back()
        v = _fp32(metric)
        best = self._value
        take = v <= best if self.mode == "min" else v >= best          # (False for a NaN)
        if take:
            sd = self.model.state_dict()
            src = [t.detach() for t in sd.values()]
            snap = self._snap if self._snap is not None else self._td_snap      # (the buffers a captured update writes, if any)
            if (snap is not None and list(snap) == list(sd)
                    and all(a.shape == b.shape and a.device == b.device and a.dtype == b.dtype for a, b in zip(snap.values(), src))):
                with torch.no_grad():
                    torch._foreach_copy_(list(snap.values()), src)
                self._snap = snap
            else:
                self._snap = OrderedDict((k, t.clone()) for k, t in zip(sd, src))
            self._value, self._best_call = v, self._calls
        self._taken = 1 if take else 0
        self._calls += 1
        self.last_path = "torch"
        # a device metric on a GPU module (or a block that a captured update already moves): keep the tensor form in step
        self._td_fresh = False
        if self._td_live or (isinstance(metric, torch.Tensor) and metric.is_cuda):
            dev = self._td_device()
            if dev is not None:
                self._td_upload(dev)
        return torch.tensor(self._taken, dtype=torch.int32)

    # ------------------------------------------------------------------ restore
    def restore(self):
        """model <- the best weights (what `torch.load` of the reference's checkpoint file gives back); raises if no snapshot
        was ever taken.  Reads the state, i.e. synchronises."""
        if self.epoch < 0:
            raise _lib.MfmError("KeepBest.restore: no snapshot was taken yet (no update call, or no metric %s the initial %g)"
                                % ("<=" if self.mode == "min" else ">=", self.initial))
        eng = self._flat_engine()
        if (eng is not None and self._on_device and self._mfm_flat.device == eng.params.device
                and self._mfm_flat.numel() == eng.layout.total):
            begin, end = eng.layout.begin, eng.layout.guard
            with torch.no_grad():
                eng.params[begin:end].copy_(self._mfm_flat[begin:end])
            return
        snap = self._flat_snapshot() if self._on_device else self._snap
        sd = self.model.state_dict()
        if list(sd) != list(snap):
            raise _lib.MfmError("KeepBest.restore: the snapshot's tensors do not match the model's state_dict")
        with torch.no_grad():
            torch._foreach_copy_([t.detach() for t in sd.values()], [snap[k].to(t.device) for k, t in sd.items()])

    # ------------------------------------------------------------------ host reads
    def _host(self):
        if self._on_device:
            self._read_back()
        self._td_read_back()
        return self

    @property
    def value(self):
        """the best metric so far (the initial value before any snapshot); synchronises on the flat path"""
        return self._host()._value

    @property
    def calls(self):
        """number of update calls so far; synchronises on the flat path"""
        return self._host()._calls

    @property
    def epoch(self):
        """0-based index of the update call that last took a snapshot, -1 if none; synchronises on the flat path"""
        return self._host()._best_call

    @property
    def taken(self):
        """whether the latest update took a snapshot; synchronises on the flat path"""
        return bool(self._host()._taken)

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """mode, initial, value, calls, epoch, taken and the snapshot (clones under the model's own parameter names, None before
        the first snapshot); synchronises on the flat path"""
        self._host()
        if self._best_call < 0:
            snap = None
        elif self._on_device:
            snap = self._flat_snapshot()
        else:
            snap = OrderedDict((k, t.clone()) for k, t in self._snap.items())
        return dict(mode=self.mode, initial=self.initial, value=self._value, calls=self._calls, epoch=self._best_call,
                    taken=self._taken, snapshot=snap)

    def load_state_dict(self, sd):
        if sd["mode"] not in _MODES:
            raise ValueError("KeepBest.load_state_dict: mode %r" % (sd["mode"],))
        snap = sd.get("snapshot")
        if snap is not None:
            want = self.model.state_dict()
            if list(snap) != list(want) or any(tuple(snap[k].shape) != tuple(want[k].shape) for k in want):
                raise _lib.MfmError("KeepBest.load_state_dict: the snapshot's tensors do not match the model's state_dict")
            snap = OrderedDict((k, snap[k].detach().to(device=want[k].device, dtype=want[k].dtype, copy=True)) for k in want)
        elif int(sd["epoch"]) >= 0:
            raise _lib.MfmError("KeepBest.load_state_dict: epoch %d but no snapshot" % int(sd["epoch"]))
        self.mode = sd["mode"]
        self.initial = _fp32(sd.get("initial", self.initial))
        self._value, self._calls, self._best_call = _fp32(sd["value"]), int(sd["calls"]), int(sd["epoch"])
        self._taken = int(sd.get("taken", 0))
        self._snap = snap
        self._on_device = False          # (the next flat call uploads state and snapshot)
        self._td_fresh = self._td_live = False
