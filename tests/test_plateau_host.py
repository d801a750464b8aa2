"""factorized_amd.lr_scheduler.ReduceLROnPlateau without a GPU: the native entry point, and the host path (the one float lrs, CPU
models and non-capturable optimizers take) against torch.optim.lr_scheduler.ReduceLROnPlateau on the same inputs -- best, the
counters, last_epoch and every group's lr compared with `==` after EVERY step -- over metric sequences built to hit the rule's
corners (`plateau_metrics`, shared with tests/test_gpu_plateau.py), checkpoints in both directions, and groups added mid-run."""
import copy
import inspect
import io
import math
import os
import re

import numpy as np
import pytest
import torch

from factorized_amd import _lib
from factorized_amd.lr_scheduler import ReduceLROnPlateau
from torch.optim.lr_scheduler import ReduceLROnPlateau as TorchPlateau

NAN, INF = float("nan"), float("inf")
STEPS = 60
THRESHOLD = 1e-4
GRID = [(mode, tmode, patience, cooldown, factor, min_lr)
        for mode in ("min", "max") for tmode in ("rel", "abs") for patience in (0, 2) for cooldown in (0, 3)
        for factor, min_lr in ((0.1, 0.0), (0.1, 1e-5), (0.5, 1e-4))]


def _f32(v):
    return float(np.float32(v))


def _bound(mode, tmode, best, threshold):
    """the value a metric has to beat, by torch's four _is_better forms (python doubles)"""
    if mode == "min":
        return best * (1.0 - threshold) if tmode == "rel" else best - threshold
    return best * (threshold + 1.0) if tmode == "rel" else best + threshold


def plateau_metrics(mode, tmode, threshold=THRESHOLD, seed=0):
    """60 fp32 metrics (python floats that are exact fp32 values), fixed seed:
      0-5    an improving prefix (6 steps)
      6      an exact tie with best
      7-9    the fp32 value one ulp on the losing side of fp32(bound), fp32(bound) itself, one ulp on the winning side, where
             bound = best * (1 - threshold) and its three siblings: the first never improves, the last always does, and
             which side fp32(bound) itself falls on is up to fp32 rounding
      10     a tie with the new best
      11     NaN          12  the infinity that is never better (+inf for min, -inf for max)
      30     another tie
      59     the infinity that always is (-inf for min, +inf for max): last, because nothing can follow it
      rest   non-improving values"""
    d = -1.0 if mode == "min" else 1.0
    rng = np.random.RandomState(1000 + seed)
    out = [_f32(5.0 + d * 0.5 * k) for k in range(6)]
    best = out[-1]
    out.append(best)
    e32 = np.float32(_bound(mode, tmode, best, threshold))
    losing, winning = np.nextafter(e32, np.float32(-d * INF)), np.nextafter(e32, np.float32(d * INF))
    out += [float(losing), float(e32), float(winning)]
    better = (lambda a, b: a < b) if mode == "min" else (lambda a, b: a > b)
    for v in out[-3:]:
        if better(v, _bound(mode, tmode, best, threshold)):
            best = v
    assert best in (float(e32), float(winning)) and not better(float(losing), _bound(mode, tmode, out[5], threshold))
    assert better(float(winning), _bound(mode, tmode, out[5], threshold))
    out += [best, NAN, -d * INF]
    while len(out) < STEPS - 1:
        out.append(best if len(out) == 30 else _f32(best - d * rng.uniform(0.1, 1.0)))
    out.append(d * INF)
    assert len(out) == STEPS and all(v != v or _f32(v) == v for v in out)
    return out


def group_lrs(n_groups):
    """starting lrs of the groups (fp32 values) and, for n_groups > 1, the index of the group whose lr tensor the LAST group
    shares (it is then reduced twice per reduction, as torch's loop does)"""
    lrs = [_f32(1e-3 * (1.0 + 0.25 * i)) if i != 1 else _f32(3e-4) for i in range(n_groups)]
    if n_groups > 1:
        lrs[-1] = lrs[0]
    return lrs, (0 if n_groups > 1 else None)


def _optimizer(lrs, shared=None, as_tensor=True, device="cpu"):
    params = [torch.nn.Parameter(torch.zeros(1)) for _ in lrs]
    opt = torch.optim.SGD([{"params": [p]} for p in params], lr=1e-3)
    tensors = [torch.tensor(v, dtype=torch.float32, device=device) for v in lrs]
    if shared is not None:
        tensors[-1] = tensors[shared]
    for g, t, v in zip(opt.param_groups, tensors, lrs):
        g["lr"] = t if as_tensor else v
    return opt


class Watch:
    """torch's class with its _reduce_lr calls classified, so that a parametrisation cannot pass by exercising nothing"""

    def __init__(self, sched):
        self.sched, self.changed, self.clamped, self.suppressed, self.bad_in_cooldown = sched, 0, 0, 0, 0
        inner = sched._reduce_lr

        def reduce_lr(epoch):
            groups = sched.optimizer.param_groups
            old = [float(g["lr"]) for g in groups]
            inner(epoch)
            new = [float(g["lr"]) for g in groups]
            self.changed += old != new
            self.suppressed += old == new
            self.clamped += any(o * sched.factor < m for o, m in zip(old, sched.min_lrs))
        sched._reduce_lr = reduce_lr

    def step(self, v):
        s = self.sched
        if s.in_cooldown and not s._is_better(float(v), s.best):
            self.bad_in_cooldown += 1
        s.step(v)

    def check(self, cooldown, factor, min_lr):
        assert self.changed >= 2
        assert cooldown == 0 or self.bad_in_cooldown >= 1
        assert min_lr == 0 or self.clamped >= 1
        assert not (min_lr == 0 and factor == 0.1) or self.suppressed >= 1


def _state(s):
    return (s.best, s.num_bad_epochs, s.cooldown_counter, s.last_epoch, [float(g["lr"]) for g in s.optimizer.param_groups])


def _same_state(mine, twin, what):
    a, b = _state(mine), _state(twin)
    assert a == b or (a[1:] == b[1:] and a[0] != a[0] and b[0] != b[0]), (what, a, b)
    for ga, gb in zip(mine.optimizer.param_groups, twin.optimizer.param_groups):
        assert type(ga["lr"]) is type(gb["lr"]), what
        if isinstance(ga["lr"], torch.Tensor):
            assert torch.equal(ga["lr"].view(torch.int32), gb["lr"].view(torch.int32)), what


# ----------------------------------------------------------------------------------- the entry point
def test_library_exports_the_entry_point_and_the_header_declares_it():
    L = _lib.lib()
    assert hasattr(L, "mfm_plateau_step") and "mfm_plateau_step" in _lib.exported_names()
    assert L.mfm_abi_version() == 5                        # (an additive entry: the ABI number stays)
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfm_hip.h")
    text = open(header).read()
    assert re.search(r"\bint\s+mfm_plateau_step\s*\(", text)
    assert "#define MFM_PLATEAU_MAX_GROUPS 16" in text and _lib.MFM_PLATEAU_MAX_GROUPS == 16
    for name in ("MIN", "MAX", "REL", "ABS"):
        assert "#define MFM_PLATEAU_%s %d" % (name, getattr(_lib, "MFM_PLATEAU_" + name)) in text
    m = re.search(r"typedef struct MfmPlateauState \{(.*?)\} MfmPlateauState;", text, re.S)
    fields = re.findall(r"\b(double|int32_t)\s+(\w+)", m.group(1))
    assert fields == [("double", "best"), ("int32_t", "num_bad_epochs"), ("int32_t", "cooldown_counter"), ("int32_t", "last_epoch"),
                      ("int32_t", "reduced"), ("int32_t", "reductions"), ("int32_t", "reserved_")]
    assert _lib.MFM_PLATEAU_STATE_WORDS * 4 == 8 + 6 * 4
    import ctypes as C
    assert C.sizeof(_lib.PlateauGroups) == 16 * 8 + 16 * 8


def test_plateau_launch_validates_on_the_host():
    """argument errors are caught before anything is enqueued (the pointers are never used)"""
    import ctypes as C
    L = _lib.lib()
    fake = (1 << 20)
    table = _lib.PlateauGroups()
    for i in range(16):
        table.lr[i] = fake + 64 + 4 * i

    def call(state=fake, metric_dev=None, groups=table, n=3, mode=0, tmode=0, factor=0.1, patience=2, cooldown=0):
        return L.mfm_plateau_step(C.c_void_p(state), C.c_void_p(metric_dev), 1.0, C.byref(groups) if groups is not None else None, n,
                                  mode, tmode, factor, 1e-4, 1e-8, patience, cooldown, -1, None)
    null_lr, odd_lr = _lib.PlateauGroups(), _lib.PlateauGroups()
    for i in range(16):
        null_lr.lr[i] = odd_lr.lr[i] = fake + 64 + 4 * i
    null_lr.lr[2] = None
    odd_lr.lr[1] = fake + 66
    cases = [(dict(state=None), b"must not be null"), (dict(groups=None), b"must not be null"),
             (dict(state=fake + 8), b"state must be 16-byte aligned"), (dict(metric_dev=fake + 2), b"device metric 4-byte aligned"),
             (dict(n=0), b"n_groups 0"), (dict(n=17), b"n_groups 17"), (dict(n=-1), b"n_groups -1"),
             (dict(groups=null_lr), b"lr pointer of group 2"), (dict(groups=odd_lr), b"lr pointer of group 1"),
             (dict(mode=2), b"unknown mode"), (dict(mode=-1), b"unknown mode"), (dict(tmode=2), b"unknown threshold mode"),
             (dict(factor=1.0), b"Factor should be < 1.0"), (dict(factor=2.5), b"Factor should be < 1.0"),
             (dict(patience=-1), b"must not be negative"), (dict(cooldown=-2), b"must not be negative")]
    for over, msg in cases:
        assert call(**over) == -1, over
        assert msg in L.mfm_last_error(), (over, L.mfm_last_error())


# ----------------------------------------------------------------------------------- signature and argument errors
def test_signature_is_torchs():
    assert inspect.signature(ReduceLROnPlateau) == inspect.signature(TorchPlateau)
    assert inspect.signature(ReduceLROnPlateau.step) == inspect.signature(TorchPlateau.step)
    assert issubclass(ReduceLROnPlateau, TorchPlateau)
    import factorized_amd.optim as optim
    assert optim.ReduceLROnPlateau is TorchPlateau and optim.lr_scheduler is torch.optim.lr_scheduler      # (unchanged aliases)


@pytest.mark.parametrize("kwargs, exc", [(dict(factor=1.0), ValueError), (dict(factor=1.5), ValueError), (dict(mode="best"), ValueError),
                                         (dict(threshold_mode="pct"), ValueError), (dict(min_lr=[0.0]), ValueError),
                                         (dict(min_lr=(0.0, 0.0, 0.0)), ValueError)])
def test_argument_errors_are_torchs(kwargs, exc):
    seen = []
    for cls in (TorchPlateau, ReduceLROnPlateau):
        with pytest.raises(exc) as info:
            cls(_optimizer([1e-3, 1e-3], as_tensor=False), **kwargs)
        seen.append(str(info.value))
    assert seen[0] == seen[1]
    with pytest.raises(TypeError, match="is not an Optimizer"):
        ReduceLROnPlateau(object())


# ----------------------------------------------------------------------------------- the host path against torch's class
@pytest.mark.parametrize("as_tensor", [False, True], ids=["float_lr", "cpu_tensor_lr"])
@pytest.mark.parametrize("mode, tmode, patience, cooldown, factor, min_lr", GRID)
def test_host_path_equals_torch_after_every_step(mode, tmode, patience, cooldown, factor, min_lr, as_tensor):
    kw = dict(mode=mode, factor=factor, patience=patience, threshold=THRESHOLD, threshold_mode=tmode, cooldown=cooldown,
              min_lr=min_lr, eps=1e-8)
    for n_groups in (1, 3, 16):
        lrs, shared = group_lrs(n_groups)
        mine = ReduceLROnPlateau(_optimizer(lrs, shared, as_tensor), **kw)
        twin = TorchPlateau(_optimizer(lrs, shared, as_tensor), **kw)
        watch = Watch(twin)
        _same_state(mine, twin, "start")
        for k, v in enumerate(plateau_metrics(mode, tmode)):
            metric = v if k % 3 else torch.tensor(v, dtype=torch.float32)           # python floats and 0-d CPU tensors
            assert mine.step(metric) is None
            watch.step(metric)
            _same_state(mine, twin, (n_groups, k, v))
            assert mine.last_path == "host" and mine.in_cooldown == twin.in_cooldown
            assert [float(a) for a in mine.get_last_lr()] == [float(b) for b in twin.get_last_lr()]
        assert mine.reductions == watch.changed and not mine.last_reduced.is_cuda
        watch.check(cooldown, factor, min_lr)
        assert math.isinf(twin.best)


def test_a_python_double_metric_keeps_its_precision():
    """torch compares python doubles: a metric that differs from best * (1 - threshold) only below fp32 resolution decides"""
    for cls in (TorchPlateau, ReduceLROnPlateau):
        s = cls(_optimizer([1e-3], as_tensor=False), patience=0, threshold=0.0)
        s.step(1.0)
        s.step(1.0 - 1e-12)                             # better in fp64, a tie in fp32
        assert s.best == 1.0 - 1e-12 and s.num_bad_epochs == 0 and s.optimizer.param_groups[0]["lr"] == 1e-3
        s.step(1.0 - 1e-12)
        assert s.optimizer.param_groups[0]["lr"] == 1e-3 * 0.1


def test_epoch_argument_is_stored_as_torch_does():
    for cls in (TorchPlateau, ReduceLROnPlateau):
        s = cls(_optimizer([1e-3], as_tensor=False))
        with pytest.warns(UserWarning):
            s.step(1.0, epoch=7)
        s.step(1.0)
        assert s.last_epoch == 8


# ----------------------------------------------------------------------------------- checkpoints
@pytest.mark.parametrize("as_tensor", [False, True], ids=["float_lr", "cpu_tensor_lr"])
def test_state_dict_goes_into_torchs_class_and_back(as_tensor):
    kw = dict(mode="min", factor=0.5, patience=2, cooldown=3, min_lr=1e-4)
    metrics = plateau_metrics("min", "rel")
    lrs, shared = group_lrs(3)
    mine, twin = ReduceLROnPlateau(_optimizer(lrs, shared, as_tensor), **kw), TorchPlateau(_optimizer(lrs, shared, as_tensor), **kw)
    for v in metrics[:20]:
        mine.step(v)
        twin.step(v)
    sd = mine.state_dict()
    assert set(sd) == set(twin.state_dict())            # torch's keys, all of them and no other
    for key in ("best", "num_bad_epochs", "cooldown_counter", "last_epoch", "mode", "factor", "patience", "threshold",
                "threshold_mode", "cooldown", "min_lrs", "eps", "_last_lr"):
        assert key in sd
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=False)
    # mine -> torch's class (different constructor arguments: everything travels), torch's -> a fresh one of mine
    into_torch = TorchPlateau(copy.deepcopy(mine.optimizer), mode="max", factor=0.9, patience=7)
    into_torch.load_state_dict(sd)
    back = ReduceLROnPlateau(copy.deepcopy(twin.optimizer), mode="max", factor=0.9, patience=7)
    back.load_state_dict(twin.state_dict())
    for s in (into_torch, back):
        _same_state(s, twin, "loaded")
        assert (s.mode, s.factor, s.patience, s.cooldown, s.min_lrs) == ("min", 0.5, 2, 3, [1e-4] * 3)
    for k, v in enumerate(metrics[20:]):
        for s in (mine, twin, into_torch, back):
            s.step(v)
        for s in (mine, into_torch, back):
            _same_state(s, twin, ("continued", k))
    clone = copy.deepcopy(mine)
    clone.step(0.0)
    assert clone.best == -INF and clone.optimizer is not mine.optimizer


# ----------------------------------------------------------------------------------- a group added mid-run
@pytest.mark.parametrize("as_tensor", [False, True], ids=["float_lr", "cpu_tensor_lr"])
def test_group_added_mid_run_with_scalar_min_lr_is_broadcast(as_tensor):
    kw = dict(factor=0.5, patience=0, min_lr=1e-4)
    metrics = plateau_metrics("min", "rel")
    mine, twin = ReduceLROnPlateau(_optimizer([1e-3, 3e-4], None, as_tensor), **kw), TorchPlateau(_optimizer([1e-3, 3e-4], None, as_tensor), **kw)
    for k, v in enumerate(metrics):
        if k == 10:
            for s in (mine, twin):
                lr = torch.tensor(2e-3) if as_tensor else 2e-3
                s.optimizer.add_param_group({"params": [torch.nn.Parameter(torch.zeros(1))], "lr": lr})
        mine.step(v)
        twin.step(v)
        _same_state(mine, twin, k)
        assert mine.min_lrs == twin.min_lrs
    assert len(mine.min_lrs) == 3 and float(mine.optimizer.param_groups[2]["lr"]) == (_f32(1e-4) if as_tensor else 1e-4)


def test_group_added_mid_run_with_list_min_lr_raises_as_torch_does():
    metrics = plateau_metrics("min", "rel")
    seen = []
    for cls in (TorchPlateau, ReduceLROnPlateau):
        s = cls(_optimizer([1e-3, 3e-4], as_tensor=False), factor=0.5, patience=0, min_lr=[1e-4, 1e-5])
        for v in metrics[:5]:
            s.step(v)
        s.optimizer.add_param_group({"params": [torch.nn.Parameter(torch.zeros(1))], "lr": 2e-3})
        s.step(metrics[5])                              # still improving: nothing is reduced, nothing is raised
        with pytest.raises(RuntimeError) as info:
            s.step(metrics[6])                          # a tie: torch reduces, and notices
        seen.append((str(info.value), s.best, s.num_bad_epochs, s.last_epoch))
    assert seen[0] == seen[1]
