"""factorized_amd.checkpoint.KeepBest on the MI355X: the keep-best kernel through the C ABI on raw buffers (poisoned
surroundings, bit-exact copies, the rule with its tie and NaN cases, the ticket that advances the state, capture), and KeepBest
in the reference's unchanged loop against a host twin kept with the reference's own lines
(`if v <= best: best = v; snap = deepcopy(state_dict)`, mfm_mosi.py:467-473): the flat path, its fallbacks, copies, checkpoints.

Every comparison of weights is bitwise: the feature copies, it computes nothing.  The one numeric bound is the project's 1e-4
relative bound on the eval-mode y_hat after restore() against a second model that got the twin's weights by load_state_dict."""
import copy
import ctypes as C
import io
import re

import numpy as np
import pytest
import torch

import factorized_amd.optim as optim
from factorized_amd import _lib, configs, swa_utils as S, synth
from factorized_amd.checkpoint import KeepBest
from tests import cases
from tests.test_gpu_sgd import _model, _reference_loop

pytestmark = pytest.mark.gpu
SENTINEL = 0x7FC0DEAD                 # a NaN with a payload: any arithmetic on it, or any store over it, shows
TILE = 1024
FULL_GRID = 2048 * TILE + TILE        # one tile more than the 2048-workgroup cap: grid-stride loop, ticket at full grid
NAN, INF = float("nan"), float("inf")
METRICS = [3.0, 2.0, 2.0, 5.0, NAN, 1.0, INF]
TAKEN = [1, 1, 1, 0, 0, 1, 0]
MODES = {"min": _lib.MFM_KEEP_MIN, "max": _lib.MFM_KEEP_MAX}
SIGN = {"min": 1.0, "max": -1.0}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _launch(best, p, begin, end, mode, metric, state):
    """metric: a device tensor (by pointer) or a python float (the scalar argument)"""
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dev, scalar = (metric, 0.0) if isinstance(metric, torch.Tensor) else (None, metric)
    _lib.check(_lib.lib().mfm_keep_best_flat(_ptr(best), _ptr(p), begin, end, mode, _ptr(dev), scalar, _ptr(state), stream),
               "mfm_keep_best_flat")


def _state(best_value, calls=0, best_call=-1):
    host = torch.zeros(_lib.MFM_KEEP_STATE_WORDS, dtype=torch.int32)
    host[0:1].view(torch.float32)[0] = best_value
    host[1], host[2] = calls, best_call
    return host.cuda()


def _read(state):
    """(best_value, calls, best_call, taken, ticket)"""
    h = state.cpu()
    return float(h[0:1].view(torch.float32)[0]), int(h[1]), int(h[2]), int(h[3]), int(h[4])


SPECIAL = torch.tensor([0x7FC00001, 0x7F800123, -0x00400000 + 0x7F, 0x7F800000, -0x00800000, 1, 0x007FFFFF, -0x7FFFFFFF, 0,
                        -0x80000000], dtype=torch.int64).to(torch.int32)
# quiet and signalling NaNs with payloads, a negative NaN, +inf, -inf, the smallest and the largest denormal, a negative
# denormal, +0 and -0


def _poisoned_pair(begin, length, seed, pad=64):
    """best, p (CPU fp32, begin + length + pad elements): N(0,1) inside [begin, begin + length) with the special bit patterns
    planted at its start, across the end of the first tile and in its last float4; the sentinel everywhere else"""
    gen = torch.Generator().manual_seed(seed)
    total = begin + length + pad
    best, p = torch.randn(total, generator=gen), torch.randn(total, generator=gen)
    inside = torch.zeros(total, dtype=torch.bool)
    inside[begin:begin + length] = True
    pv = p.view(torch.int32)
    pv[begin:begin + 4] = SPECIAL[:4]
    pv[begin + length - 2:begin + length] = SPECIAL[-2:]
    if length >= 1020 + SPECIAL.numel():
        pv[begin + 1020:begin + 1020 + SPECIAL.numel() - 2] = SPECIAL[:-2]
    for t in (best, p):
        t.view(torch.int32)[~inside] = SENTINEL
    return best, p, inside


def _metric_form(form, v):
    return torch.tensor(v, dtype=torch.float32, device="cuda") if form == "device" else v


@pytest.mark.parametrize("form", ["device", "scalar"])
@pytest.mark.parametrize("taken", [True, False])
@pytest.mark.parametrize("begin", [0, 64])
@pytest.mark.parametrize("length", [4, 1020, 1024, 1028, 3 * 1024 + 4])
def test_kernel_copies_bit_for_bit_or_not_at_all_and_touches_nothing_outside(length, begin, taken, form):
    _need_gpu()
    best0, p0, inside = _poisoned_pair(begin, length, seed=length + begin)
    best, p, state = best0.cuda(), p0.cuda(), _state(4.0, calls=6, best_call=2)
    metric = 3.5 if taken else 4.5
    _launch(best, p, begin, begin + length, _lib.MFM_KEEP_MIN, _metric_form(form, metric), state)
    assert _read(state) == ((3.5, 7, 6, 1, 0) if taken else (4.0, 7, 2, 0, 0))
    assert torch.equal(_bits(p), _bits(p0))                                    # p is never written
    assert torch.equal(_bits(best)[~inside], _bits(best0)[~inside])            # the canaries around the range
    want = p0 if taken else best0
    assert torch.equal(_bits(best)[inside], _bits(want)[inside])               # NaN payloads and -0.0 included


@pytest.mark.parametrize("form", ["device", "scalar"])
@pytest.mark.parametrize("mode", list(MODES))
def test_rule_ties_take_and_nan_never_takes(mode, form):
    _need_gpu()
    s = SIGN[mode]
    best0, p0, inside = _poisoned_pair(64, 1028, seed=11)
    #        best_value, metric, taken
    table = [(s * 2.0, s * 2.0, 1),            # a tie takes (the reference's <=)
             (s * 2.0, s * 1.0, 1), (s * 2.0, s * 3.0, 0),
             (s * 2.0, NAN, 0), (s * INF, NAN, 0), (NAN, s * 1.0, 0),          # a NaN on either side never takes
             (s * INF, s * INF, 1),                                            # inf <= inf: the first call with the default start
             (s * INF, s * 999999.0, 1), (-s * INF, s * 1.0, 0),
             (0.0, -0.0, 1), (-0.0, 0.0, 1)]
    for best_value, metric, taken in table:
        best, p, state = best0.cuda(), p0.cuda(), _state(best_value, calls=3, best_call=1)
        _launch(best, p, 64, 64 + 1028, MODES[mode], _metric_form(form, metric), state)
        got = _read(state)
        assert got[1:] == (4, 3 if taken else 1, taken, 0), (best_value, metric, got)
        kept = metric if taken else best_value
        assert np.float32(got[0]).tobytes() == np.float32(kept).tobytes() or (kept != kept and got[0] != got[0])
        assert torch.equal(_bits(best), _bits(p0 if taken else best0) * inside + _bits(best0) * ~inside)
        assert torch.equal(_bits(p), _bits(p0))


@pytest.mark.parametrize("taken", [True, False])
def test_kernel_over_more_tiles_than_workgroups(taken):
    _need_gpu()
    best0, p0, inside = _poisoned_pair(64, FULL_GRID, seed=3)
    best, p, state = best0.cuda(), p0.cuda(), _state(INF)
    _launch(best, p, 64, 64 + FULL_GRID, _lib.MFM_KEEP_MIN, 1.0 if taken else NAN, state)
    assert _read(state) == ((1.0, 1, 0, 1, 0) if taken else (INF, 1, -1, 0, 0))
    want = torch.where(inside, _bits(p0), _bits(best0)) if taken else _bits(best0)
    assert torch.equal(_bits(best), want)
    assert torch.equal(_bits(p), _bits(p0))


@pytest.mark.parametrize("length", [TILE, FULL_GRID], ids=["one_workgroup", "full_grid"])
def test_ticket_advances_the_state_once_per_launch(length):
    _need_gpu()
    best0, p0, inside = _poisoned_pair(0, length, seed=6)
    best, p, state = best0.cuda(), p0.cuda(), _state(INF)
    held = None
    for i, (metric, best_call, taken, value) in enumerate([(5.0, 0, 1, 5.0), (7.0, 0, 0, 5.0), (5.0, 2, 1, 5.0), (4.0, 3, 1, 4.0)]):
        form = metric if i % 2 else torch.tensor(metric, device="cuda")
        _launch(best, p, 0, length, _lib.MFM_KEEP_MIN, form, state)
        assert _read(state) == (value, i + 1, best_call, taken, 0)
        if taken:
            held = p[:length].clone()
        assert torch.equal(best[:length].view(torch.int32), held.view(torch.int32))
        p[:length] += 0.25
    assert torch.equal(_bits(best)[~inside], _bits(best0)[~inside])


def test_launch_replays_from_a_captured_graph_and_decides_anew():
    _need_gpu()
    begin, length = 64, 3 * 1024 + 4
    best0, p0, inside = _poisoned_pair(begin, length, seed=7)
    warm = _state(INF)
    _launch(best0.cuda(), p0.cuda(), begin, begin + length, _lib.MFM_KEEP_MIN, 1.0, warm)      # (the code object is loaded)
    best, p, state = best0.cuda(), p0.cuda(), _state(INF)
    metric = torch.zeros((), device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _launch(best, p, begin, begin + length, _lib.MFM_KEEP_MIN, metric, state)
    assert _read(state) == (INF, 0, -1, 0, 0) and torch.equal(_bits(best), _bits(best0))      # (captured, not run)
    held = None
    for i, (v, value, best_call, taken) in enumerate([(10.0, 10.0, 0, 1), (5.0, 5.0, 1, 1), (7.0, 5.0, 1, 0)]):
        metric.fill_(v)
        graph.replay()
        torch.cuda.synchronize()
        assert _read(state) == (value, i + 1, best_call, taken, 0)
        if taken:
            held = _bits(p)
        assert torch.equal(_bits(best)[inside], held[inside])
        assert torch.equal(_bits(best)[~inside], _bits(best0)[~inside])
        p[begin:begin + length] += 0.5


# ----------------------------------------------------------------------------------- the reference loop
B, T_STEPS = 5, 7


def _setup(cls="MFM_KL_EF", seed=7):
    cfgs = configs.canonical_configs(dropout=False)
    model = _model(cfgs, cls=cls)
    optimizer = optim.Adam(model.parameters())                     # before .to(device), as in the reference
    model = model.to("cuda")
    xn, yn = synth.make_batch(cfgs[0]["input_dims"], B, T_STEPS, seed=seed)
    return model, optimizer, torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda(), cfgs[0]


def _step(model, optimizer, X, y, cfg, n=1):
    _reference_loop(model, optimizer, X, y, cfg, n)


class Twin:
    """the reference's lines, on the host"""

    def __init__(self, model, mode="min", best=INF):
        self.model, self.mode, self.best, self.snap, self.epoch, self.calls = model, mode, best, None, -1, 0

    def update(self, v):
        take = v <= self.best if self.mode == "min" else v >= self.best
        if take:
            self.best = v
            self.snap = copy.deepcopy(self.model.state_dict())
            self.epoch = self.calls
        self.calls += 1
        return take


def _same(sd_a, sd_b, what=None):
    assert list(sd_a) == list(sd_b), what
    for k in sd_a:
        assert torch.equal(_bits(sd_a[k]), _bits(sd_b[k])), (what, k)


def _dev(v):
    return torch.tensor(v, dtype=torch.float32, device="cuda")


def _check_against_twin(kb, twin, took, what):
    assert int(took) == int(twin.calls and twin.epoch == twin.calls - 1), what
    assert (kb.calls, kb.epoch) == (twin.calls, twin.epoch), what
    assert kb.value == twin.best, what
    snap = kb.state_dict()["snapshot"]
    assert (snap is None) == (twin.snap is None), what
    if snap is not None:
        _same(snap, twin.snap, what)


def _eval_y(model, X):
    model.eval()
    with torch.no_grad():
        decoded, _, _ = model(X)
    model.train()
    return decoded[3].detach().cpu().numpy()


def _keepbest_run(cls, mode="min"):
    s = SIGN[mode]
    model, optimizer, X, y, cfg = _setup(cls)
    _step(model, optimizer, X, y, cfg)                   # (the model is on its engine from its first forward on)
    kb, twin = KeepBest(model, mode=mode), Twin(model, mode, s * INF)
    taken = []
    for k, v in enumerate(METRICS):
        _step(model, optimizer, X, y, cfg, 2)
        took = kb.update(_dev(s * v))
        assert kb.last_path == "flat" and took.is_cuda and took.dim() == 0 and took.dtype == torch.int32
        twin.update(s * v)
        _check_against_twin(kb, twin, took, (cls, mode, k))
        taken.append(int(took))
    assert taken == TAKEN and kb.epoch == 5
    _step(model, optimizer, X, y, cfg, 2)
    assert not torch.equal(_bits(model._plist[0]), _bits(twin.snap[model._param_names[0]]))
    kb.restore()
    _same(model.state_dict(), twin.snap, (cls, "restore"))
    assert model._flat_ok() and model._grad_views_attached()
    second = _model(configs.canonical_configs(dropout=False), cls=cls).to("cuda")
    second.load_state_dict(copy.deepcopy(twin.snap))
    got, want = _eval_y(model, X), _eval_y(second, X)
    err = cases.rel_err(got, want)
    cases.report("keepbest_restore_yhat_rel_%s" % cls, err)
    print("keepbest_restore_yhat_rel_%s %.3e" % (cls, err))
    assert err < 1e-4, (cls, err)
    _step(model, optimizer, X, y, cfg)                   # training goes on from the restored weights
    assert model._flat_ok() and optimizer._fallback is None


@pytest.mark.parametrize("mode", ["min", "max"])
def test_unchanged_loop_snapshots_follow_the_host_twin_bit_for_bit(mode):
    _need_gpu()
    _keepbest_run("MFM_KL_EF", mode)


def test_mfm_kl_and_its_104_tensors():
    _need_gpu()
    assert len(_model(configs.canonical_configs(dropout=False), cls="MFM_KL")._plist) == 104
    _keepbest_run("MFM_KL")


def test_mfm():
    _need_gpu()
    _keepbest_run("MFM")


def test_flat_path_does_not_synchronise_or_allocate_after_the_first_call():
    _need_gpu()
    model, optimizer, X, y, cfg = _setup()
    _step(model, optimizer, X, y, cfg)
    kb = KeepBest(model)
    metrics = [_dev(v) for v in (3.0, 2.0, 4.0)]
    with pytest.raises(_lib.MfmError, match="no snapshot"):
        kb.restore()
    kb.update(metrics[0])                               # (first call: snapshot buffer and state block are allocated)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        took = [kb.update(metrics[1]), kb.update(metrics[2]), kb.update(1.5)]          # device, device, a python float
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert took[0] is took[1] and int(took[2]) == 1     # (a view of live state: it shows the latest call)
    assert (kb.calls, kb.epoch, kb.value, kb.taken) == (4, 3, 1.5, True)
    assert int(kb._mfm_ticket) == 0


def test_loss_expr_and_other_metric_forms():
    _need_gpu()
    from factorized_amd import lazy
    model, optimizer, X, y, cfg = _setup()
    _step(model, optimizer, X, y, cfg)
    kb = KeepBest(model, initial=999999.0)
    assert int(kb.update(NAN)) == 0                     # (first call: buffers and state are set up, with an upload)
    model.train()
    decoded, mmd_loss, _ = model(X)
    assert isinstance(mmd_loss, lazy.LossExpr)
    expr = 2.0 * mmd_loss + 1.0
    want = expr.item()
    torch.cuda.set_sync_debug_mode("error")
    try:
        took = kb.update(expr)                          # evaluated on the device: no read-back
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert kb.last_path == "flat" and int(took) == 1
    assert abs(kb.value - want) <= 1e-6 * abs(want)
    assert int(kb.update(torch.tensor(kb.value))) == 1                      # a CPU tensor, a tie
    assert int(kb.update(torch.tensor([kb.value - 1.0], dtype=torch.float64, device="cuda"))) == 1      # fp64 on the device
    assert int(kb.update(_dev(kb.value + 1.0).reshape(1, 1))) == 0
    assert kb.calls == 5 and kb.epoch == 3
    with pytest.raises(ValueError):
        kb.update(torch.zeros(2, device="cuda"))


def test_update_inside_a_capture_takes_device_metrics_only():
    _need_gpu()
    model, optimizer, X, y, cfg = _setup()
    _step(model, optimizer, X, y, cfg)
    kb, twin = KeepBest(model), Twin(model)
    metric = torch.zeros((), device="cuda")
    fresh = KeepBest(model)
    kb.update(_dev(50.0))                               # (first call outside the capture: buffers; the code object is loaded)
    twin.update(50.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kb.update(metric)
        with pytest.raises(_lib.MfmError, match="baked into the graph"):
            kb.update(3.0)
        with pytest.raises(_lib.MfmError, match="baked into the graph"):
            kb.update(torch.tensor(3.0))
        with pytest.raises(_lib.MfmError, match="outside the stream capture"):
            fresh.update(metric)
    assert kb.calls == 1
    for k, v in enumerate([10.0, 5.0, 7.0]):
        _step(model, optimizer, X, y, cfg)
        metric.fill_(v)
        graph.replay()
        twin.update(v)
        _check_against_twin(kb, twin, kb._mfm_taken, ("replay", k))
    assert (kb.calls, kb.epoch, kb.value) == (4, 2, 5.0)


def _whole(text):
    return "^" + re.escape(text) + "$"


def test_metric_arg_of_the_flat_utilities():
    """_flat.metric_arg, the metric resolution KeepBest.update and ReduceLROnPlateau.step share (no launch of the library)"""
    _need_gpu()
    from factorized_amd import _flat
    dev = torch.device("cuda", torch.cuda.current_device())
    who, where = "KeepBest.update", "the model's device"
    # a 0-d fp32 tensor on the device goes in by its own pointer: no copy
    own = torch.tensor(0.75, device=dev)
    keep, host = _flat.metric_arg(own, dev, who, where)
    assert host is None and keep.data_ptr() == own.data_ptr() and keep.dtype == torch.float32 and keep.dim() == 0
    # a 1-element fp64 device tensor: fp32 on the device, rounded to nearest
    wide = torch.tensor([1.0 + 2.0 ** -24 + 2.0 ** -40], dtype=torch.float64, device=dev)      # just above the midpoint: rounds up
    keep, host = _flat.metric_arg(wide, dev, who, where)
    assert host is None and keep.dtype == torch.float32 and keep.device == dev and keep.numel() == 1
    assert float(keep) == 1.0 + 2.0 ** -23
    # more than one element is refused with the caller's name in front
    # (the whole text, by `match`: an ExceptionInfo kept in a local would tie this frame, and the graph below, into a cycle)
    with pytest.raises(ValueError, match=_whole("KeepBest.update: the metric must have one element, not shape (2,)")):
        _flat.metric_arg(torch.zeros(2, device=dev), dev, who, where)
    # a host float inside a capture is refused; the capture ends cleanly and the graph replays
    buf = torch.zeros(1, device=dev)
    text = ("ReduceLROnPlateau.step: a host metric (python float or CPU tensor) inside a stream capture would be baked into the "
            "graph -- every replay would compare the same number.  Pass the metric as a 0-d fp32 tensor on the learning rates' "
            "device")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # (captures on a side stream of its own)
        assert _flat.capturing()
        buf.add_(1.0)
        with pytest.raises(_lib.MfmError, match=_whole(text)):
            _flat.metric_arg(3.0, dev, "ReduceLROnPlateau.step", "the learning rates' device")
    assert not _flat.capturing()
    graph.replay()
    assert float(buf) == 1.0
    assert _flat.metric_arg(3.0, dev, who, where) == (None, 3.0)


def test_composed_and_frozen_models_take_the_torch_path_and_equal_the_twin():
    _need_gpu()
    from factorized_amd import mfm_extra as X_
    torch.manual_seed(3)
    composed = X_.M_A(*configs.canonical_configs(dropout=False)).cuda()
    model, optimizer, X, y, cfg = _setup()
    _step(model, optimizer, X, y, cfg)
    assert model._flat_ok()
    model._plist[3].requires_grad_(False)               # a frozen parameter: on its flat buffer, yet the torch path here
    for m in (composed, model):
        kb, twin = KeepBest(m), Twin(m)
        for k, v in enumerate(METRICS):
            with torch.no_grad():
                for p in m.parameters():
                    p.add_(0.01 * (k + 1))
            took = kb.update(_dev(v) if k % 2 else v)
            assert kb.last_path == "torch" and not took.is_cuda
            twin.update(v)
            _check_against_twin(kb, twin, took, (type(m).__name__, k))
        with torch.no_grad():
            next(m.parameters()).add_(1.0)
        kb.restore()
        _same(m.state_dict(), twin.snap)


def test_flat_and_torch_paths_alternate_on_one_instance():
    _need_gpu()
    model, optimizer, X, y, cfg = _setup()
    _step(model, optimizer, X, y, cfg)
    kb, twin = KeepBest(model), Twin(model)
    frozen = model._plist[3]
    paths = []
    for k, v in enumerate(METRICS):
        _step(model, optimizer, X, y, cfg)
        frozen.requires_grad_(k % 2 == 0)                # odd calls: a frozen parameter sends the call to the torch path
        took = kb.update(_dev(v))
        paths.append(kb.last_path)
        twin.update(v)
        _check_against_twin(kb, twin, took, ("alternate", k))
        frozen.requires_grad_(True)
    assert paths == ["flat", "torch"] * 3 + ["flat"]
    # a model off its flat buffer (a .to() round trip, no forward since): the torch path, with the state carried over
    model.fast_grads = False
    model.to("cpu")
    model.to("cuda")
    assert not model._flat_ok()
    with torch.no_grad():
        model._plist[0].add_(1.0)
    took = kb.update(0.5)
    twin.update(0.5)
    assert kb.last_path == "torch"
    _check_against_twin(kb, twin, took, "off the flat buffer")
    with torch.no_grad():
        model._plist[0].add_(1.0)
    kb.restore()
    _same(model.state_dict(), twin.snap)


def test_update_after_optimizer_steps_and_from_an_averaged_module():
    _need_gpu()
    model, optimizer, X, y, cfg = _setup()
    _step(model, optimizer, X, y, cfg)
    ema = S.AveragedModel(model, multi_avg_fn=S.get_ema_multi_avg_fn(0.9))
    ema.update_parameters(model)
    kb, twin = KeepBest(model), Twin(model)
    kb_ema, twin_ema = KeepBest(ema.module), Twin(ema.module)
    for k, v in enumerate(METRICS):
        _step(model, optimizer, X, y, cfg)              # optim.Adam's fused step moves the flat buffer
        ema.update_parameters(model)
        for b, t in ((kb, twin), (kb_ema, twin_ema)):
            took = b.update(_dev(v))
            assert b.last_path == "flat"
            t.update(v)
            _check_against_twin(b, t, took, ("adam / ema", k))
    assert optimizer._fallback is None and model._handover_ok()
    kb_ema.restore()
    _same(ema.module.state_dict(), twin_ema.snap)
    assert not torch.equal(_bits(kb._mfm_flat), _bits(kb_ema._mfm_flat))


def test_checkpoint_into_a_fresh_instance_continues_the_sequence():
    _need_gpu()
    model, optimizer, X, y, cfg = _setup()
    _step(model, optimizer, X, y, cfg)
    kb, twin = KeepBest(model), Twin(model)
    for v in METRICS[:3]:
        _step(model, optimizer, X, y, cfg)
        kb.update(_dev(v))
        twin.update(v)
    buf = io.BytesIO()
    torch.save({"model": model.state_dict(), "best": kb.state_dict()}, buf)
    buf.seek(0)
    ck = torch.load(buf, weights_only=False)
    assert list(ck["best"]["snapshot"]) == list(model.state_dict()) and not any("ticket" in k for k in ck["best"])
    model2, optimizer2, _, _, _ = _setup()
    model2.load_state_dict(ck["model"])
    _step(model2, optimizer2, X, y, cfg)                 # (on its engine)
    fresh = KeepBest(model2, mode="max")
    fresh.load_state_dict(ck["best"])
    twin2 = Twin(model2)
    twin2.best, twin2.snap, twin2.epoch, twin2.calls = twin.best, copy.deepcopy(twin.snap), twin.epoch, twin.calls
    clone = copy.deepcopy(kb)                            # (its model is a copy off its engine: the torch path)
    assert clone._mfm_ticket is None and kb._mfm_ticket is not None
    for k, v in enumerate(METRICS[3:]):
        _step(model, optimizer, X, y, cfg)
        _step(model2, optimizer2, X, y, cfg)
        for b, t in ((kb, twin), (fresh, twin2)):
            took = b.update(_dev(v))
            assert b.last_path == "flat"
            t.update(v)
            _check_against_twin(b, t, took, ("continued", k))
        clone.update(v)
    assert (fresh.calls, fresh.epoch, fresh.value) == (kb.calls, kb.epoch, kb.value) == (7, 5, 1.0)
    assert (clone.calls, clone.epoch, clone.value) == (7, 5, 1.0) and clone.last_path == "torch"
