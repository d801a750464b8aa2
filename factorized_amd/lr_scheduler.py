"""ReduceLROnPlateau without leaving the device: what the reference's end-of-epoch line does through the host
(mfm_mosi.py:470-477, the same in mfm_you.py / mfm_moud.py / mfm_mmmo.py)

    valid_loss = evaluate(model, X_valid, y_valid)
    scheduler.step(valid_loss)            # ReduceLROnPlateau(optimizer, 'min')

keeps its two lines; only the import changes:

    from factorized_amd.lr_scheduler import ReduceLROnPlateau      # instead of torch.optim.lr_scheduler's
    scheduler = ReduceLROnPlateau(optimizer, 'min')
    ...
    scheduler.step(valid_loss)     # python float, 0-d tensor (CPU or device), or a lazy LossExpr

Signature, argument errors, attributes (`best`, `num_bad_epochs`, `cooldown_counter`, `last_epoch`, `in_cooldown`,
`get_last_lr()`), `state_dict()` keys and the rule are torch 2.10's `torch.optim.lr_scheduler.ReduceLROnPlateau`, whose subclass
this is (an `isinstance` test in a training loop keeps working); a checkpoint moves between the two classes in both
directions.  `factorized_amd.optim.ReduceLROnPlateau` stays torch's own class.

Device path.  torch's `step()` begins with `float(metrics)` and its `_reduce_lr` reads a tensor lr back with
`float(param_group["lr"])`: two host synchronisations that keep the epoch tail out of a stream capture.  When every
`param_group["lr"]` is a 1-element fp32 tensor on one and the same GPU and there are at most 16 groups -- what
`optim.Adam(..., lr=tensor, capturable=True)` and `torch.optim.Adam(..., lr=tensor, capturable=True)` hold, so the `.opt` of
`train.GraphedModuleStep` and `train.GraphedStep` qualify; only the lr tensors matter, not the optimizer class -- `step(metric)`
is ONE launch of `mfm_plateau_step` (csrc/plateau.hip) on the current stream: metric, rule, state and the lr words stay in
device memory.

  * No host synchronisation and no allocation: the state block is allocated at construction.  A 0-d or 1-element fp32 tensor
    on that GPU goes in by pointer (another dtype or device is converted to fp32 on the device first); a `LossExpr` is
    evaluated to such a tensor by the kernels that materialise its value anywhere else; a python float or a CPU tensor goes in
    as the launch's double argument and keeps torch's full precision.
  * The kernel evaluates torch's expressions in fp64 without contraction, so its decisions, its state and the bits of every lr
    equal what torch's class computes from the same metrics and lrs.
  * Inside a stream capture only the device form is accepted: a host value would be baked into the graph and every replay
    would compare the same number, so `_lib.MfmError` is raised.  A replayed launch decides anew.  The hyper-parameters
    (`factor`, `patience`, `threshold`, `cooldown`, `min_lrs`, `eps`, the modes) and the lr pointers are arguments of the launch:
    a captured step keeps the ones it was captured with.
  * `step()` returns None, as torch's.  `last_reduced` is a 0-d int32 view of the state's `reduced` word (1: the latest step
    changed at least one lr): reading it is the caller's choice, and the next step overwrites it.  `best`, `num_bad_epochs`,
    `cooldown_counter`, `last_epoch`, `in_cooldown`, `reductions`, `state_dict()` read the state back, i.e. synchronise;
    `get_last_lr()` / `_last_lr` are clones of the lr tensors, as torch keeps them.
  * Eligibility is checked on every call (pointer, dtype and device checks).  When a group's lr has become a float, a group
    was added that does not qualify, or there are more than 16 groups, the state is read back once and the instance goes on
    on the host path; when the lrs qualify again the state is uploaded (outside a stream capture only).  `last_path` says
    which path the latest step took: "device" or "host".
  * `step(metric, epoch=k)`, torch's deprecated form, stores k; k = -1 is the launch's word for "last_epoch + 1" and is refused.

Host path.  Everything else -- float lrs, CPU models, SGD, the non-capturable optimizers -- runs the same rule in python doubles
on host state and writes lrs the way torch does (`fill_` on a tensor lr, assignment otherwise): its results equal torch's class
on the same inputs, and it is always available.  A `len(param_groups) != len(min_lrs)` is handled as torch does when an lr is
about to be reduced: RuntimeError if `min_lr` was given as a list, otherwise the scalar is broadcast (the device path broadcasts
the scalar at the step that sees the new group; a list that no longer fits sends the step to the host path and its error).

Data parallel: ranks that pass the same metric (the all-reduced validation loss) take the same decisions from the same rule,
so the replicas' learning rates stay in step without any communication; no collective is involved."""
import ctypes as C
import warnings
from math import inf

import torch
from torch.optim import Optimizer
from torch.optim.lr_scheduler import EPOCH_DEPRECATION_WARNING
from torch.optim.lr_scheduler import ReduceLROnPlateau as _TorchReduceLROnPlateau

from . import _flat, _lib

__all__ = ["ReduceLROnPlateau"]

_MODES = {"min": _lib.MFM_PLATEAU_MIN, "max": _lib.MFM_PLATEAU_MAX}
_THRESHOLD_MODES = {"rel": _lib.MFM_PLATEAU_REL, "abs": _lib.MFM_PLATEAU_ABS}
# MfmPlateauState as int32 words (best: the double in words 0-1); _STATE: the words of the host form, in the order of _read_back
_W_BEST, _W_BAD, _W_COOLDOWN, _W_EPOCH, _W_REDUCED, _W_REDUCTIONS = 0, 2, 3, 4, 5, 6
_STATE = ((_W_BEST, "float64"),) + tuple((w, "int32") for w in (_W_BAD, _W_COOLDOWN, _W_EPOCH, _W_REDUCED, _W_REDUCTIONS))
_INT32_MAX = 2 ** 31 - 1


def _host_state(name):
    """an attribute of torch's class whose value lives in the device state block while the device path is in use: reading
    synchronises, writing (as `load_state_dict` and `_reset` do) hands the state back to the host until the next step"""
    field = "_h_" + name

    def get(self):
        if self._on_device:
            self._read_back()
        return getattr(self, field)

    def put(self, value):
        if self.__dict__.get("_on_device"):
            self._read_back()
            self._on_device = False
        setattr(self, field, value)

    return property(get, put)


class ReduceLROnPlateau(_TorchReduceLROnPlateau):
    """torch.optim.lr_scheduler.ReduceLROnPlateau whose step is one launch when the learning rates are device tensors (see the
    module doc)."""

    best = _host_state("best")
    num_bad_epochs = _host_state("num_bad_epochs")
    cooldown_counter = _host_state("cooldown_counter")
    last_epoch = _host_state("last_epoch")

    def __init__(self, optimizer: "Optimizer", mode: "Literal['min', 'max']" = "min", factor: "float" = 0.1,  # noqa: F821
                 patience: "int" = 10, threshold: "float" = 1e-4, threshold_mode: "Literal['rel', 'abs']" = "rel",  # noqa: F821
                 cooldown: "int" = 0, min_lr: "list[float] | float" = 0, eps: "float" = 1e-8) -> "None":
        # torch's checks, in its order and with its messages
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        self.factor = factor
        if not isinstance(optimizer, Optimizer):
            raise TypeError(f"{type(optimizer).__name__} is not an Optimizer")
        self.optimizer = optimizer
        if isinstance(min_lr, (list, tuple)):
            if len(min_lr) != len(optimizer.param_groups):
                raise ValueError(f"expected {len(optimizer.param_groups)} min_lrs, got {len(min_lr)}")
            self.default_min_lr = None
            self.min_lrs = list(min_lr)
        else:
            self.default_min_lr = min_lr
            self.min_lrs = [min_lr] * len(optimizer.param_groups)
        self.patience = patience
        self.cooldown = cooldown
        self.eps = eps
        self.last_path = None            # "device" / "host": the path of the latest step
        # device form of the state (authoritative while _on_device is True)
        self._on_device = False
        self._mfm_state = None           # int32[MFM_PLATEAU_STATE_WORDS] beside the lr tensors
        self._mfm_reduced = None         # its `reduced` word (a 0-d view: last_reduced)
        self._mfm_table = None           # (key, PlateauGroups): the launch's table, rebuilt when a pointer or a min_lr changes
        # host form (authoritative while _on_device is False)
        self._h_reduced, self._h_reductions = 0, 0
        self.last_epoch = 0
        self._h_last_lr = self._lr_list()
        self._init_is_better(mode=mode, threshold=threshold, threshold_mode=threshold_mode)
        self._reset()
        lrs = self._device_lrs()
        if lrs is not None and not _flat.capturing():
            self._to_device(lrs[0].device)          # (the state block is allocated here, not in the first step)

    # ------------------------------------------------------------------ copies
    def __getstate__(self):
        state = dict(self.__dict__)
        state["_mfm_table"] = None               # (pointers of this process; rebuilt by the next step)
        state["_mfm_reduced"] = None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        if self._mfm_state is not None:
            self._mfm_reduced = self._mfm_state[_W_REDUCED]

    # ------------------------------------------------------------------ which path
    def _device_lrs(self):
        """the groups' lr tensors if the device path can take them, else None (cheap: type, dtype and device checks)"""
        groups = self.optimizer.param_groups
        n = len(groups)
        if not 1 <= n <= _lib.MFM_PLATEAU_MAX_GROUPS or (n != len(self.min_lrs) and self.default_min_lr is None):
            return None
        lrs, dev = [], None
        for g in groups:
            lr = g["lr"]
            if not (isinstance(lr, torch.Tensor) and lr.is_cuda and lr.dtype == torch.float32 and lr.numel() == 1):
                return None
            if dev is None:
                dev = lr.device
            elif lr.device != dev:
                return None
            lrs.append(lr)
        return lrs

    def _lr_list(self):
        """torch's _param_groups_val_list(optimizer, "lr"): tensors as clones, so the list never aliases a live lr"""
        return [g["lr"].clone() if isinstance(g["lr"], torch.Tensor) else g["lr"] for g in self.optimizer.param_groups]

    # ------------------------------------------------------------------ hand-over between the two forms of the state
    def _to_device(self, dev):
        """the host state into the block beside the lr tensors (construction, or the first device step after host steps)"""
        if self._on_device and self._mfm_state.device == dev:
            return
        if _flat.capturing():
            raise _lib.MfmError("ReduceLROnPlateau.step: the scheduler's state is on the host (it stepped on the host path, or "
                                "was loaded or changed there) and is uploaded by the next step on the device path; make that "
                                "step outside the stream capture")
        if self._on_device:                      # the lr tensors moved to another GPU: carry the state over
            self._read_back()
            self._on_device = False
        ints = (self._h_num_bad_epochs, self._h_cooldown_counter, self._h_last_epoch)
        if not all(isinstance(v, int) and -_INT32_MAX <= v < _INT32_MAX for v in ints):
            raise _lib.MfmError("ReduceLROnPlateau: num_bad_epochs, cooldown_counter and last_epoch must be int32 values for "
                                "the device path, not %r" % (ints,))
        values = (float(self._h_best),) + ints + (self._h_reduced, self._h_reductions)
        host = _flat.pack_words(_lib.MFM_PLATEAU_STATE_WORDS, [(w, kind, v) for (w, kind), v in zip(_STATE, values)])
        if self._mfm_state is None or self._mfm_state.device != dev:
            self._mfm_state = host.to(dev)
            self._mfm_reduced = self._mfm_state[_W_REDUCED]
        else:
            self._mfm_state.copy_(host)
        self._on_device = True

    def _read_back(self):
        """the device state into the host fields (synchronises); the device form stays authoritative"""
        (self._h_best, self._h_num_bad_epochs, self._h_cooldown_counter, self._h_last_epoch, self._h_reduced,
         self._h_reductions) = _flat.unpack_words(self._mfm_state.cpu(), _STATE)

    def _to_host(self):
        if self._on_device:
            self._read_back()
            self._on_device = False

    def _table(self, lrs):
        n = len(lrs)
        if n != len(self.min_lrs):               # (torch's broadcast of a scalar min_lr over a changed number of groups)
            self.min_lrs = [self.default_min_lr] * n
        key = (tuple(t.data_ptr() for t in lrs), tuple(self.min_lrs))
        if self._mfm_table is None or self._mfm_table[0] != key:
            tab = _lib.PlateauGroups()
            for i, (ptr, floor) in enumerate(zip(*key)):
                tab.lr[i], tab.min_lr[i] = ptr, float(floor)
            self._mfm_table = (key, tab)
        return self._mfm_table[1]

    # ------------------------------------------------------------------ step
    def step(self, metrics: "SupportsFloat", epoch=None) -> "None":  # noqa: F821
        """torch's step(); on the device path one launch, no synchronisation (see the module doc)"""
        lrs = self._device_lrs()
        if lrs is None:
            return self._step_host(metrics, epoch)
        dev = lrs[0].device
        # (keep: alive over the launch; a host metric keeps the double)
        keep, host = _flat.metric_arg(metrics, dev, "ReduceLROnPlateau.step", "the learning rates' device")
        ptr, scalar = (keep.data_ptr(), 0.0) if keep is not None else (None, host)
        if epoch is None:
            epoch = -1
        else:
            warnings.warn(EPOCH_DEPRECATION_WARNING, UserWarning, stacklevel=2)
            if not isinstance(epoch, int) or epoch == -1 or not -_INT32_MAX <= epoch < _INT32_MAX:
                raise ValueError("ReduceLROnPlateau.step: on the device path `epoch` must be an int32 other than -1, not %r"
                                 % (epoch,))
        self._to_device(dev)
        table = self._table(lrs)
        if torch.cuda.current_device() != dev.index:
            with torch.cuda.device(dev):
                self._launch(ptr, scalar, table, len(lrs), epoch, dev)
        else:
            self._launch(ptr, scalar, table, len(lrs), epoch, dev)
        self.last_path = "device"

    def _launch(self, ptr, scalar, table, n, epoch, dev):
        _lib.check(_lib.lib().mfm_plateau_step(C.c_void_p(self._mfm_state.data_ptr()), C.c_void_p(ptr), scalar, C.byref(table), n,
                                               _MODES[self.mode], _THRESHOLD_MODES[self.threshold_mode], self.factor,
                                               self.threshold, self.eps, self.patience, self.cooldown, epoch,
                                               _flat.stream_ptr(dev)), "mfm_plateau_step")

    def _step_host(self, metrics, epoch):
        """torch 2.10's step / _is_better / _reduce_lr, statement for statement (the rule csrc/plateau.hip restates)"""
        self._to_host()
        current = float(metrics)
        if epoch is None:
            epoch = self._h_last_epoch + 1
        else:
            warnings.warn(EPOCH_DEPRECATION_WARNING, UserWarning, stacklevel=3)
        self._h_last_epoch = epoch
        if self._is_better(current, self._h_best):
            self._h_best = current
            self._h_num_bad_epochs = 0
        else:
            self._h_num_bad_epochs += 1
        if self._h_cooldown_counter > 0:
            self._h_cooldown_counter -= 1
            self._h_num_bad_epochs = 0
        self._h_reduced = 0
        if self._h_num_bad_epochs > self.patience:
            self._reduce_lr(epoch)
            self._h_cooldown_counter = self.cooldown
            self._h_num_bad_epochs = 0
        self._h_reductions += self._h_reduced
        self._h_last_lr = self._lr_list()
        self.last_path = "host"

    def _reduce_lr(self, epoch):
        groups = self.optimizer.param_groups
        if len(groups) != len(self.min_lrs):
            if self.default_min_lr is None:
                raise RuntimeError("The number of param groups in the `optimizer` "
                                   f"({len(groups)}) differs "
                                   f"from when `ReduceLROnPlateau` was initialized "
                                   f"({len(self.min_lrs)}), usually due to a new "
                                   "param group being added to the optimizer. Please "
                                   "modify the `min_lrs` field to match the length "
                                   "of the `optimizer` param groups.")
            self.min_lrs = [self.default_min_lr] * len(groups)
        for i, param_group in enumerate(groups):
            old_lr = float(param_group["lr"])
            new_lr = max(old_lr * self.factor, self.min_lrs[i])
            if old_lr - new_lr > self.eps:
                if isinstance(param_group["lr"], torch.Tensor):
                    param_group["lr"].fill_(new_lr)
                else:
                    param_group["lr"] = new_lr
                self._h_reduced = 1

    def _is_better(self, a, best):
        if self.mode == "min" and self.threshold_mode == "rel":
            rel_epsilon = 1.0 - self.threshold
            return a < best * rel_epsilon
        elif self.mode == "min" and self.threshold_mode == "abs":
            return a < best - self.threshold
        elif self.mode == "max" and self.threshold_mode == "rel":
            rel_epsilon = self.threshold + 1.0
            return a > best * rel_epsilon
        else:
            return a > best + self.threshold

    def _init_is_better(self, mode, threshold, threshold_mode):
        if mode not in {"min", "max"}:
            raise ValueError("mode " + mode + " is unknown!")
        if threshold_mode not in {"rel", "abs"}:
            raise ValueError("threshold mode " + threshold_mode + " is unknown!")
        self.mode_worse = inf if mode == "min" else -inf
        self.mode = mode
        self.threshold = threshold
        self.threshold_mode = threshold_mode

    def _reset(self):
        """Reset num_bad_epochs counter and cooldown counter."""
        self.best = self.mode_worse
        self.cooldown_counter = 0
        self.num_bad_epochs = 0

    # ------------------------------------------------------------------ reads
    @property
    def in_cooldown(self):
        return self.cooldown_counter > 0

    @property
    def last_reduced(self):
        """0-d int32: 1 if the latest step changed at least one lr.  Device path: a view of device state (no synchronisation
        until it is read; the next step overwrites it)."""
        if self._on_device:
            return self._mfm_reduced
        return torch.tensor(self._h_reduced, dtype=torch.int32)

    @property
    def reductions(self):
        """number of steps so far that changed at least one lr; synchronises on the device path"""
        if self._on_device:
            self._read_back()
        return self._h_reductions

    @property
    def _last_lr(self):
        """device path: clones of the lr tensors as they are now (the step keeps no list: that would allocate); host path:
        the list torch keeps, taken at the end of the latest step"""
        return self._lr_list() if self._on_device else self._h_last_lr

    @_last_lr.setter
    def _last_lr(self, value):
        self._h_last_lr = value

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """torch's keys (every attribute of torch's class but the optimizer); synchronises on the device path"""
        if self._on_device:
            self._read_back()
        return dict(factor=self.factor, default_min_lr=self.default_min_lr, min_lrs=list(self.min_lrs), patience=self.patience,
                    cooldown=self.cooldown, eps=self.eps, last_epoch=self._h_last_epoch, _last_lr=self._last_lr,
                    mode_worse=self.mode_worse, mode=self.mode, threshold=self.threshold, threshold_mode=self.threshold_mode,
                    best=self._h_best, cooldown_counter=self._h_cooldown_counter, num_bad_epochs=self._h_num_bad_epochs)

    def load_state_dict(self, state_dict):
        """a state_dict of this class or of torch's; the next step on the device path uploads it"""
        self._to_host()
        for key, value in state_dict.items():
            setattr(self, key, value)
        self._init_is_better(mode=self.mode, threshold=self.threshold, threshold_mode=self.threshold_mode)
