"""factorized_amd.lr_scheduler.ReduceLROnPlateau on the MI355X: the plateau kernel through the C ABI against torch's own class on
CPU fp32 tensor lrs (state block and every lr word compared for BIT EQUALITY after every one of 60 steps: the kernel evaluates
torch's fp64 expressions without contraction, and `fill_` rounds as `(float)` does, so tolerance 0 is the right bar), guard
words around state and lrs, launches that must not write, the launcher's refusals; and the scheduler in the reference's
unchanged loop, under hipGraph replay, across its host / device hand-overs and through checkpoints, against a twin run with
torch's scheduler fed `.item()` values.

The one numeric bound is the project's 1e-4 relative bound on the parameters of two separately trained models (the KeepBest
twin test's); lrs are compared bit for bit."""
import copy
import ctypes as C
import io

import numpy as np
import pytest
import torch

import factorized_amd.optim as optim
from factorized_amd import _lib, configs, synth
from factorized_amd.checkpoint import KeepBest
from factorized_amd.lr_scheduler import ReduceLROnPlateau
from tests import cases
from tests.test_gpu_sgd import _model, _reference_loop
from tests.test_plateau_host import GRID, THRESHOLD, TorchPlateau, Watch, _optimizer, group_lrs, plateau_metrics

pytestmark = pytest.mark.gpu
SENTINEL = 0x7FA0DEAD                 # a SIGNALLING NaN with a payload: any conversion of it, or any store over it, shows
NAN, INF = float("nan"), float("inf")
MODES = {"min": _lib.MFM_PLATEAU_MIN, "max": _lib.MFM_PLATEAU_MAX}
TMODES = {"rel": _lib.MFM_PLATEAU_REL, "abs": _lib.MFM_PLATEAU_ABS}
GUARD = 4                             # int32 words on either side of the state block (keeps it 16-byte aligned)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(v):
    return torch.tensor(v, dtype=torch.float32, device="cuda")


class Block:
    """state block and lr words in device memory, each between guard words:
    state buffer  [GUARD x sentinel | MfmPlateauState | GUARD x sentinel]
    lr buffer     [sentinel, lr_0, sentinel, lr_1, ..., lr_{n-1}, sentinel]   (group i: word 1 + 2 i)"""

    def __init__(self, mode, lrs, shared=None):
        host = torch.full((2 * GUARD + _lib.MFM_PLATEAU_STATE_WORDS,), SENTINEL, dtype=torch.int32)
        host[GUARD:GUARD + 8] = 0
        host[GUARD:GUARD + 2].view(torch.float64)[0] = INF if mode == "min" else -INF
        self.state = host.cuda()
        words = torch.full((2 * len(lrs) + 1,), SENTINEL, dtype=torch.int32)
        words[1::2] = torch.tensor(lrs, dtype=torch.float32).view(torch.int32)
        self.index = [1 + 2 * i for i in range(len(lrs))]
        if shared is not None:
            words[self.index[-1]] = SENTINEL             # (its own word is never used: it must keep the sentinel)
            self.index[-1] = self.index[shared]
        self.lr = words.cuda()
        self.table = _lib.PlateauGroups()
        self.n = len(lrs)

    def state_ptr(self):
        return self.state.data_ptr() + 4 * GUARD

    def fill_table(self, min_lrs):
        for i, (w, m) in enumerate(zip(self.index, min_lrs)):
            self.table.lr[i], self.table.min_lr[i] = self.lr.data_ptr() + 4 * w, m

    def read(self):
        """(best, num_bad_epochs, cooldown_counter, last_epoch, reduced, reductions), the lr words of the groups as int32 bits"""
        s, w = self.state.cpu(), self.lr.cpu()
        assert (s[:GUARD] == SENTINEL).all() and (s[GUARD + 8:] == SENTINEL).all() and int(s[GUARD + 7]) == 0
        unused = torch.ones_like(w, dtype=torch.bool)
        unused[self.index] = False
        assert (w[unused] == SENTINEL).all()             # the guards, and the word of a group that shares another's tensor
        st = s[GUARD:GUARD + 8]
        return (float(st[0:2].view(torch.float64)[0]),) + tuple(int(v) for v in st[2:7]), w[self.index]


def _launch(blk, metric, mode, tmode, factor, patience, cooldown, n=None, state_ptr=None, threshold=THRESHOLD, eps=1e-8, epoch=-1,
            table=None):
    """metric: a device tensor (by pointer) or a python float (the double argument); returns the launcher's code"""
    dev, scalar = (metric.data_ptr(), 0.0) if isinstance(metric, torch.Tensor) else (None, metric)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return _lib.lib().mfm_plateau_step(C.c_void_p(blk.state_ptr() if state_ptr is None else state_ptr), C.c_void_p(dev), scalar,
                                       C.byref(blk.table if table is None else table), blk.n if n is None else n, mode, tmode,
                                       factor, threshold, eps, patience, cooldown, epoch, stream)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _twin_state(twin):
    return (twin.best, twin.num_bad_epochs, twin.cooldown_counter, twin.last_epoch)


def _same_best(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


# ----------------------------------------------------------------------------------- the kernel through the C ABI
@pytest.mark.parametrize("mode, tmode, patience, cooldown, factor, min_lr", GRID)
def test_kernel_equals_torch_bit_for_bit_after_every_step(mode, tmode, patience, cooldown, factor, min_lr):
    _need_gpu()
    metrics = plateau_metrics(mode, tmode)
    for n_groups in (1, 3, 16):
        lrs, shared = group_lrs(n_groups)
        for form in ("device", "scalar"):
            blk = Block(mode, lrs, shared)
            blk.fill_table([min_lr] * n_groups)
            twin = TorchPlateau(_optimizer(lrs, shared), mode=mode, factor=factor, patience=patience, threshold=THRESHOLD,
                                threshold_mode=tmode, cooldown=cooldown, min_lr=min_lr, eps=1e-8)
            watch, reductions = Watch(twin), 0
            for k, v in enumerate(metrics):
                before = blk.read()[1]
                changed = watch.changed
                rc = _launch(blk, _dev(v) if form == "device" else v, MODES[mode], TMODES[tmode], factor, patience, cooldown)
                assert rc == 0, _lib.lib().mfm_last_error()
                watch.step(torch.tensor(v, dtype=torch.float32) if form == "device" else v)
                state, words = blk.read()
                what = (n_groups, form, k, v, state, _twin_state(twin))
                assert _same_best(state[0], twin.best) and state[1:4] == _twin_state(twin)[1:], what
                want = torch.cat([_bits(g["lr"]).reshape(1) for g in twin.optimizer.param_groups])
                assert torch.equal(words, want), what
                reduced = int(watch.changed != changed)
                reductions += reduced
                assert state[4:] == (reduced, reductions), what
                if not reduced:
                    assert torch.equal(words, before), what          # a launch that does not reduce leaves every lr word alone
            watch.check(cooldown, factor, min_lr)


def test_an_lr_the_rule_leaves_alone_is_not_rewritten():
    """old - new > eps is false for a NaN lr: its word keeps its bits (a signalling NaN would come back quiet from any store of
    a converted value), while the groups around it are reduced; the same for an lr already at its floor"""
    _need_gpu()
    lrs = [1e-3, 1e-3, 1e-4, 1e-3]
    blk = Block("min", lrs)
    blk.fill_table([0.0, 0.0, 1e-4, 0.0])
    words = blk.lr.cpu()
    words[blk.index[1]] = SENTINEL
    blk.lr.copy_(words)
    floor_bits = int(words[blk.index[2]])
    for k, v in enumerate([1.0, 1.0, 1.0]):
        assert _launch(blk, _dev(v), 0, 0, 0.1, 0, 0) == 0
        state, got = blk.read()
        assert int(got[1]) == SENTINEL and int(got[2]) == floor_bits
        assert state[4] == (1 if k else 0) and state[5] == k
    want = np.float32(float(np.float32(float(np.float32(1e-3)) * 0.1)) * 0.1)          # two reductions, each rounded to fp32
    assert torch.equal(got[[0, 3]], torch.tensor([want, want], dtype=torch.float32).view(torch.int32))


def test_epoch_argument_and_entries_above_n_groups():
    _need_gpu()
    blk = Block("max", [1e-3, 2e-3, 4e-3])
    blk.fill_table([0.0, 0.0, 0.0])
    blk.table.lr[2] = None                              # not looked at while n_groups == 2: group 2 keeps its lr
    assert _launch(blk, 1.0, 1, 1, 0.5, 0, 0, n=2, epoch=41) == 0
    assert _launch(blk, 1.0, 1, 1, 0.5, 0, 0, n=2) == 0
    state, got = blk.read()
    assert state == (1.0, 0, 0, 42, 1, 1)
    assert torch.equal(got, torch.tensor([5e-4, 1e-3, 4e-3], dtype=torch.float32).view(torch.int32))


def test_launcher_refusals_leave_state_and_lrs_untouched():
    _need_gpu()
    blk = Block("min", [1e-3, 3e-4, 1e-3])
    blk.fill_table([0.0] * 3)
    assert _launch(blk, 2.0, 0, 0, 0.1, 0, 0) == 0 and _launch(blk, 2.0, 0, 0, 0.1, 0, 0) == 0       # (a state worth keeping)
    state0, lr0 = blk.state.cpu(), blk.lr.cpu()
    null_lr, odd_lr = _lib.PlateauGroups(), _lib.PlateauGroups()
    for i in range(3):
        null_lr.lr[i] = odd_lr.lr[i] = blk.table.lr[i]
    null_lr.lr[1] = None
    odd_lr.lr[2] = blk.table.lr[2] + 2
    refusals = [(dict(state_ptr=0), b"must not be null"), (dict(state_ptr=blk.state_ptr() + 4), b"state must be 16-byte aligned"),
                (dict(state_ptr=blk.state_ptr() + 8), b"state must be 16-byte aligned"),
                (dict(n=0), b"n_groups 0"), (dict(n=17), b"n_groups 17"), (dict(table=null_lr), b"lr pointer of group 1"),
                (dict(table=odd_lr), b"lr pointer of group 2"), (dict(mode=2), b"unknown mode"), (dict(tmode=3), b"unknown threshold mode"),
                (dict(factor=1.0), b"Factor should be < 1.0"), (dict(patience=-1), b"must not be negative"),
                (dict(cooldown=-1), b"must not be negative")]
    for over, msg in refusals:
        kw = dict(mode=0, tmode=0, factor=0.1, patience=0, cooldown=0)
        kw.update(over)
        for metric in (_dev(3.0), 3.0):
            assert _launch(blk, metric, **kw) == -1, over
            assert msg in _lib.lib().mfm_last_error(), (over, _lib.lib().mfm_last_error())
    torch.cuda.synchronize()
    assert torch.equal(blk.state.cpu(), state0) and torch.equal(blk.lr.cpu(), lr0)


# ----------------------------------------------------------------------------------- the scheduler class on device lrs
def _pair(lrs, shared=None, **kw):
    """ReduceLROnPlateau on device lr tensors and torch's class on CPU tensors holding the same values"""
    mine = ReduceLROnPlateau(_optimizer(lrs, shared, device="cuda"), **kw)
    twin = TorchPlateau(_optimizer(lrs, shared), **kw)
    return mine, twin


def _follows(mine, twin, what):
    assert _same_best(mine.best, twin.best), what
    assert (mine.num_bad_epochs, mine.cooldown_counter, mine.last_epoch, mine.in_cooldown) == \
        (twin.num_bad_epochs, twin.cooldown_counter, twin.last_epoch, twin.in_cooldown), what
    for a, b in zip(mine.optimizer.param_groups, twin.optimizer.param_groups):
        la, lb = a["lr"], b["lr"]
        la = _bits(la) if torch.is_tensor(la) else torch.tensor(la, dtype=torch.float64)
        lb = _bits(lb) if torch.is_tensor(lb) else torch.tensor(lb, dtype=torch.float64)
        assert la.dtype == lb.dtype and torch.equal(la.reshape(-1), lb.reshape(-1)), what


def test_device_path_does_not_synchronise_or_allocate_and_takes_every_metric_form():
    _need_gpu()
    kw = dict(mode="min", factor=0.5, patience=1, cooldown=1, min_lr=1e-4)
    lrs, shared = group_lrs(3)
    mine, twin = _pair(lrs, shared, **kw)
    assert mine._on_device and mine._mfm_state is not None          # allocated at construction
    metrics = plateau_metrics("min", "rel")
    forms = [_dev(v) if k % 3 == 0 else (_dev(v).reshape(1, 1) if k % 3 == 1 else v) for k, v in enumerate(metrics)]
    mine.step(forms[0])                                  # (the code object is loaded)
    twin.step(metrics[0])
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for k in range(1, 40):
            assert mine.step(forms[k]) is None and mine.last_path == "device"
            flag = mine.last_reduced
            assert flag.is_cuda and flag.dim() == 0 and flag.dtype == torch.int32
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    watch = Watch(twin)
    for k in range(1, 40):
        watch.step(metrics[k])
    _follows(mine, twin, "40 steps")
    assert mine.reductions == watch.changed >= 2
    # converted on the device: an fp64 device tensor, a CPU tensor; more than one element is refused
    mine.step(torch.tensor([metrics[40]], dtype=torch.float64, device="cuda"))
    mine.step(torch.tensor(metrics[41]))
    twin.step(metrics[40])
    twin.step(metrics[41])
    _follows(mine, twin, "converted")
    with pytest.raises(ValueError):
        mine.step(torch.zeros(2, device="cuda"))
    with pytest.warns(UserWarning):
        mine.step(_dev(metrics[42]), epoch=70)
    with pytest.warns(UserWarning):
        twin.step(metrics[42], epoch=70)
    _follows(mine, twin, "epoch=")
    assert [float(v) for v in mine.get_last_lr()] == [float(v) for v in twin.get_last_lr()]


def test_hand_over_between_device_and_host_paths():
    _need_gpu()
    kw = dict(mode="min", factor=0.5, patience=0, cooldown=0, min_lr=0.0)
    metrics = plateau_metrics("min", "rel")
    mine, twin = _pair([1e-3, 3e-4], **kw)
    paths = []
    for k, v in enumerate(metrics[:30]):
        if k == 8:                                       # a group's tensor lr becomes a float: the host path takes over
            for s in (mine, twin):
                s.optimizer.param_groups[1]["lr"] = float(s.optimizer.param_groups[1]["lr"])
        if k == 16:                                      # ... and a tensor comes back: the state is uploaded again
            mine.optimizer.param_groups[1]["lr"] = _dev(mine.optimizer.param_groups[1]["lr"])
            twin.optimizer.param_groups[1]["lr"] = torch.tensor(twin.optimizer.param_groups[1]["lr"], dtype=torch.float32)
        mine.step(_dev(v))
        twin.step(v)
        paths.append(mine.last_path)
        _follows(mine, twin, ("float and back", k))
    assert paths == ["device"] * 8 + ["host"] * 8 + ["device"] * 14
    # a 17th group: more than the launch's table holds
    lrs, shared = group_lrs(16)
    mine, twin = _pair(lrs, shared, **kw)
    paths = []
    for k, v in enumerate(metrics[:20]):
        if k == 9:
            mine.optimizer.add_param_group({"params": [torch.nn.Parameter(torch.zeros(1))], "lr": _dev(2e-3)})
            twin.optimizer.add_param_group({"params": [torch.nn.Parameter(torch.zeros(1))], "lr": torch.tensor(2e-3)})
        mine.step(_dev(v))
        twin.step(v)
        paths.append(mine.last_path)
        _follows(mine, twin, ("17 groups", k))
    assert paths == ["device"] * 9 + ["host"] * 11 and len(mine.min_lrs) == len(twin.min_lrs) == 17


def test_checkpoint_from_the_device_path_into_a_fresh_instance_and_into_torchs_class():
    _need_gpu()
    kw = dict(mode="max", factor=0.1, patience=2, cooldown=3, min_lr=1e-5, threshold_mode="abs")
    metrics = plateau_metrics("max", "abs")
    lrs, shared = group_lrs(3)
    mine, twin = _pair(lrs, shared, **kw)
    for v in metrics[:20]:
        mine.step(_dev(v))
        twin.step(v)
    assert mine.last_path == "device"
    buf = io.BytesIO()
    torch.save(mine.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=False)
    assert set(sd) == set(twin.state_dict())
    now = [float(g["lr"]) for g in mine.optimizer.param_groups]
    fresh = ReduceLROnPlateau(_optimizer(now, shared, device="cuda"), mode="min", factor=0.9)
    into_torch = TorchPlateau(_optimizer(now, shared), mode="min", factor=0.9)
    fresh.load_state_dict(copy.deepcopy(sd))
    into_torch.load_state_dict(copy.deepcopy(sd))
    clone = copy.deepcopy(mine)                          # (its own optimizer, lr tensors and state block)
    for k, v in enumerate(metrics[20:]):
        for s in (mine, fresh, clone):
            s.step(_dev(v))
            assert s.last_path == "device"
        twin.step(v)
        into_torch.step(v)
        for s in (mine, fresh, clone, into_torch):
            _follows(s, twin, ("continued", k))
    assert clone._mfm_state.data_ptr() != mine._mfm_state.data_ptr()


# ----------------------------------------------------------------------------------- the reference loop
B, T_STEPS, EPOCHS, STEPS_PER_EPOCH = 5, 3, 6, 2


def _batch(cfg):
    xn, yn = synth.make_batch(cfg["input_dims"], B, T_STEPS, seed=7)
    return torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()


def _param_err(a, b):
    return max(cases.rel_err(p.detach().cpu().numpy(), q.detach().cpu().numpy()) for p, q in zip(a.parameters(), b.parameters()))


def _valid_loss(model, X):
    """evaluate(): a forward on the validation batch whose loss stays a lazy expression of device values"""
    model.train()
    decoded, mmd_loss, _ = model(X)
    return 2.0 * mmd_loss + 1.0


@pytest.mark.parametrize("mode", ["min", "max"])
def test_unchanged_loop_epoch_tail_runs_without_a_sync_and_follows_the_torch_twin(mode):
    _need_gpu()
    from factorized_amd import lazy
    cfgs = configs.canonical_configs(dropout=False)
    cfg = cfgs[0]
    X, y = _batch(cfg)
    runs = []
    for which in ("device", "twin"):
        model = _model(cfgs).to("cuda")
        lr = torch.tensor([1e-3], device="cuda")
        optimizer = optim.Adam(model.parameters(), lr=lr, capturable=True)
        cls = ReduceLROnPlateau if which == "device" else TorchPlateau
        scheduler = cls(optimizer, mode, patience=0)
        best = KeepBest(model)
        _reference_loop(model, optimizer, X, y, cfg, 1)          # (on its engine; every code object loaded)
        trajectory = []
        for epoch in range(EPOCHS):
            _reference_loop(model, optimizer, X, y, cfg, STEPS_PER_EPOCH)
            valid_loss = _valid_loss(model, X)
            assert isinstance(valid_loss, lazy.LossExpr)
            if which == "device":
                if epoch == 0:
                    scheduler.step(valid_loss)           # (the kernels that materialise a LossExpr are loaded)
                    best.update(valid_loss)
                else:
                    torch.cuda.set_sync_debug_mode("error")
                    try:
                        scheduler.step(valid_loss)
                        best.update(valid_loss)
                    finally:
                        torch.cuda.set_sync_debug_mode("default")
                assert scheduler.last_path == "device" and best.last_path == "flat"
            else:
                v = valid_loss.item()
                scheduler.step(v)
                best.update(v)
            trajectory.append(int(_bits(lr)))
        print("plateau_loop_%s_%s lr %s best %r" % (mode, which, [float(np.int32(b).view(np.float32)) for b in trajectory],
                                                    scheduler.best))
        runs.append((model, scheduler, trajectory, best))
    (m_dev, s_dev, t_dev, kb_dev), (m_twin, s_twin, t_twin, kb_twin) = runs
    assert t_dev == t_twin                               # the lr, bit for bit, after every epoch
    assert (s_dev.num_bad_epochs, s_dev.cooldown_counter, s_dev.last_epoch) == (s_twin.num_bad_epochs, s_twin.cooldown_counter,
                                                                                s_twin.last_epoch) and s_dev.last_epoch == EPOCHS
    assert abs(s_dev.best - s_twin.best) <= 1e-6 * abs(s_twin.best)          # (a LossExpr's device value is fp32, .item() a double)
    if mode == "max":
        assert s_dev.reductions >= 4                     # the loss falls: every epoch after the first is a bad one
    err = _param_err(m_dev, m_twin)
    cases.report("plateau_loop_param_rel_%s" % mode, err)
    print("plateau_loop_param_rel_%s %.3e" % (mode, err))
    assert err < 1e-4, err


def _graphed_run(which, make, steps_of):
    """EPOCHS epochs of STEPS_PER_EPOCH replayed steps, each followed by scheduler.step(loss of the last step)"""
    gs, params = make()
    scheduler = (ReduceLROnPlateau if which == "device" else TorchPlateau)(gs.opt, "max", patience=0)
    trajectory = []
    for epoch in range(EPOCHS):
        for _ in range(STEPS_PER_EPOCH):
            loss = steps_of(gs)
        if which == "device":
            if epoch == 0:
                scheduler.step(loss)
            else:
                torch.cuda.set_sync_debug_mode("error")
                try:
                    scheduler.step(loss)
                finally:
                    torch.cuda.set_sync_debug_mode("default")
            assert scheduler.last_path == "device"
        else:
            scheduler.step(loss.item())
        trajectory.append(int(_bits(gs.lr)))
    return scheduler, trajectory, params


def _graphed_pair(make, steps_of, name, reproducible=True):
    (s_dev, t_dev, p_dev), (s_twin, t_twin, p_twin) = [_graphed_run(w, make, steps_of) for w in ("device", "twin")]
    print("plateau_graphed_%s lr %s" % (name, [float(np.int32(b).view(np.float32)) for b in t_dev]))
    assert t_dev == t_twin and s_dev.reductions >= 4
    assert (s_dev.num_bad_epochs, s_dev.cooldown_counter, s_dev.last_epoch) == (s_twin.num_bad_epochs, s_twin.cooldown_counter,
                                                                                s_twin.last_epoch)
    if not reproducible:
        return
    err = max(cases.rel_err(p.detach().cpu().numpy(), q.detach().cpu().numpy()) for p, q in zip(p_dev, p_twin))
    cases.report("plateau_graphed_param_rel_%s" % name, err)
    print("plateau_graphed_param_rel_%s %.3e" % (name, err))
    assert err < 1e-4, err


def test_graphed_module_step_optimizer_takes_the_device_path():
    _need_gpu()
    from factorized_amd import train
    cfgs = configs.canonical_configs(dropout=False)
    X, y = _batch(cfgs[0])

    def make():
        model = _model(cfgs).to("cuda")
        gs = train.GraphedModuleStep(model, cfgs[0], B, T_STEPS, lr=1e-3)
        assert gs.fused and isinstance(gs.opt, optim.Adam)
        return gs, list(model.parameters())
    _graphed_pair(make, lambda gs: gs.step(X, y)[0], "module_step")


def test_torch_adam_capturable_on_a_composed_model_takes_the_device_path():
    """lr trajectory (bit for bit) and scheduler state against the torch twin.  The parameters of the two runs are NOT compared:
    training of a composed model is not reproducible from run to run (its module-path backward sums with atomics, and Adam turns
    the last bits of a small gradient into a full step).  Measured on the MI355X with no code of this feature in the loop: two
    runs of this very twin with torch's own scheduler end 0.128 apart (worst tensor, last_to_zy_fc1.weight, relative), two runs
    at a constant lr without any scheduler 0.282; the second training step's loss already differs in the third digit.  A bound
    on that difference would measure the model's kernels, not the scheduler.  The fused model of the test above is
    reproducible, and there the parameters are held to 1e-4."""
    _need_gpu()
    from factorized_amd import mfm_extra, train
    cfgs = configs.canonical_configs(dropout=False)
    X, _ = _batch(cfgs[0])

    def objective(out):
        ts = []

        def flat(o):
            if torch.is_tensor(o):
                ts.append(o)
            elif isinstance(o, (list, tuple)):
                for q in o:
                    flat(q)
        flat(out)
        return sum((t * t).mean() if t.dim() else t for t in ts if t.dtype.is_floating_point)

    def make():
        torch.manual_seed(3)
        model = mfm_extra.M_A(*cfgs).cuda()
        model.train()
        gen = torch.Generator().manual_seed(5)          # (the MMD prior samples: fixed, or the two runs train on different draws)
        model.mmd_gauss = [torch.randn(B, cfgs[0][k], generator=gen).cuda() for k in ("zl_size", "zy_size")]
        gs = train.GraphedStep(model, lambda m, x: objective(m.forward(x)), [X], lr=1e-3)
        assert type(gs.opt) is torch.optim.Adam
        return gs, list(model.parameters())
    _graphed_pair(make, lambda gs: gs.step(X), "composed", reproducible=False)


# ----------------------------------------------------------------------------------- capture
def test_step_and_keepbest_update_captured_in_one_graph_follow_the_twin_on_every_replay():
    _need_gpu()
    from tests.test_gpu_keepbest import Twin, _setup, _step
    model, optimizer, X, y, cfg = _setup()
    _step(model, optimizer, X, y, cfg)
    kw = dict(mode="min", factor=0.5, patience=1, cooldown=1, min_lr=1e-4)
    lrs, shared = group_lrs(3)
    mine, twin = _pair(lrs, shared, **kw)
    kb, kb_twin = KeepBest(model), Twin(model)
    metrics = plateau_metrics("min", "rel")
    metric = torch.zeros((), device="cuda")
    metric.fill_(metrics[0])
    mine.step(metric)                                    # (outside the capture: code objects; KeepBest's buffers)
    kb.update(metric)
    twin.step(metrics[0])
    kb_twin.update(metrics[0])
    host_only = ReduceLROnPlateau(_optimizer(lrs, shared, device="cuda"), **kw)
    host_only.best = 3.0                                 # (its state is on the host until the next step uploads it)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mine.step(metric)
        kb.update(metric)
        with pytest.raises(_lib.MfmError, match="baked into the graph"):
            mine.step(3.0)
        with pytest.raises(_lib.MfmError, match="baked into the graph"):
            mine.step(torch.tensor(3.0))
        with pytest.raises(_lib.MfmError, match="outside the stream capture"):
            host_only.step(metric)
    _follows(mine, twin, "captured, not run")
    for k in range(1, 13):                               # 12 replays, a new metric in the static tensor each time
        _step(model, optimizer, X, y, cfg)
        v = metrics[k + 4]                               # (from the end of the improving prefix on: ties, the bound, NaN, inf)
        metric.fill_(v)
        graph.replay()
        twin.step(v)
        kb_twin.update(v)
        _follows(mine, twin, ("replay", k, v))
        assert (kb.calls, kb.epoch) == (kb_twin.calls, kb_twin.epoch) and (kb.value == kb_twin.best or v != v)
    assert mine.reductions >= 2 and mine.last_epoch == 13
