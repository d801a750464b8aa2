"""factorized_amd.swa_utils on the MI355X: the averaging kernel through the C ABI against torch.lerp on raw buffers (poisoned
surroundings, the bit-exact first copy, the ticket that advances the count, capture), and AveragedModel in the reference's
unchanged loop against torch's class on twins: the flat path, its fallbacks, copies and checkpoints.

The yardstick is torch.optim.swa_utils.AveragedModel itself, run at test time.  The bound of every comparison with it is
k * 2^-21 * max(|avg|, |p|) after k lerp updates: two fp32 roundings per update on either side, fused or unfused multiply-add."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.optim.swa_utils as T

import factorized_amd.optim as optim
from factorized_amd import _lib, configs, swa_utils as S, synth
from tests import cases
from tests.test_gpu_sgd import _model, _reference_loop

pytestmark = pytest.mark.gpu
SENTINEL = 0x7FC0DEAD                 # a NaN with a payload: any arithmetic on it, or any store over it, shows
ULP_BOUND = 2.0 ** -21
TILE = 1024
FULL_GRID = 2049 * TILE               # one tile more than the 2048-workgroup cap: grid-stride loop, ticket at full grid
KINDS = {"swa": _lib.MFM_AVG_SWA, "ema": _lib.MFM_AVG_EMA}
DECAY = 0.9


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _launch(avg, p, begin, end, kind, w, n, ticket):
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().mfm_avg_flat(_ptr(avg), _ptr(p), begin, end, kind, w, _ptr(n), _ptr(ticket), stream), "mfm_avg_flat")


def _poisoned_pair(begin, length, seed, pad=64):
    """avg, p (CPU fp32, begin + length + pad elements): N(0,1) in [begin, begin + length), the sentinel everywhere else; and
    the mask of the inside"""
    gen = torch.Generator().manual_seed(seed)
    total = begin + length + pad
    avg, p = torch.randn(total, generator=gen), torch.randn(total, generator=gen)
    inside = torch.zeros(total, dtype=torch.bool)
    inside[begin:begin + length] = True
    for t in (avg, p):
        t.view(torch.int32)[~inside] = SENTINEL
    return avg, p, inside


def _state(n0):
    return torch.full((), n0, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")


def _torch_weight(kind, n):
    """the lerp weight as torch's multi_avg_fn forms it: SWA from the int64 count tensor, EMA a Python scalar"""
    return 1 / (n + 1) if kind == "swa" else 1 - DECAY


def _five_updates(kind, begin, length, seed):
    """five lerp updates (n = 1 .. 5; the source moves between them) by the kernel and by torch.lerp on the same device ->
    worst |difference| inside the range, its bound, and the final buffers for the checks outside the range"""
    avg0, p0, inside = _poisoned_pair(begin, length, seed)
    avg, p, ref = avg0.cuda(), p0.cuda(), avg0.cuda()[begin:begin + length].clone()
    n, ticket = _state(1)
    n_ref = torch.full((), 1, dtype=torch.int64, device="cuda")
    scale = max(float(avg0[inside].abs().max()), float(p0[inside].abs().max()) + 0.4)      # (the source moves by 4 x 0.1)
    worst = 0.0
    for k in range(5):
        if k:
            p[begin:begin + length] += 0.1            # (inside only: the sentinels outside stay)
        _launch(avg, p, begin, begin + length, KINDS[kind], 1.0 - DECAY, n, ticket)
        ref = torch.lerp(ref, p[begin:begin + length], _torch_weight(kind, n_ref))
        n_ref += 1
        worst = max(worst, float((avg[begin:begin + length] - ref).abs().max()))
        assert int(n) == k + 2 and int(ticket) == 0
    p_want = p0.clone()
    for _ in range(4):
        p_want[inside] += 0.1
    return worst, 5 * ULP_BOUND * scale, avg.cpu(), avg0, p.cpu(), p_want, inside, ref.cpu()


def _assert_within(worst, bound, key):
    """worst |kernel - torch.lerp| over the five updates against k * 2^-21 * max(|avg|, |p|), k = 5.

    Measured worst difference on the MI355X: not measured yet (no GPU run was possible when this was written); every run
    prints and records it.  Once it is measured as 0 for every case, this becomes a bitwise comparison."""
    cases.report(key, worst)
    print("%s worst %.3e (bound %.3e)" % (key, worst, bound))
    assert worst < bound, (key, worst, bound)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("begin", [0, 64])
@pytest.mark.parametrize("length", [4, 1020, 1024, 1028, 3 * 1024 + 4])
def test_kernel_matches_torch_lerp_and_touches_nothing_outside(length, begin, kind):
    _need_gpu()
    worst, bound, avg, avg0, p, p_want, inside, ref = _five_updates(kind, begin, length, seed=length + begin)
    _assert_within(worst, bound, "swa_kernel_abs_%s_%d_%d" % (kind, begin, length))
    assert torch.equal(_bits(avg)[~inside], _bits(avg0)[~inside])          # nothing outside the range was written
    assert torch.equal(_bits(p), _bits(p_want))                            # p is never written
    assert bool(torch.isfinite(avg[inside]).all())                         # ... and no sentinel was read into the range


@pytest.mark.parametrize("kind", list(KINDS))
def test_kernel_over_more_tiles_than_workgroups(kind):
    _need_gpu()
    worst, bound, avg, avg0, p, p_want, inside, ref = _five_updates(kind, 64, FULL_GRID, seed=3)
    _assert_within(worst, bound, "swa_kernel_abs_%s_full_grid" % kind)
    assert torch.equal(_bits(avg)[~inside], _bits(avg0)[~inside])
    assert torch.equal(_bits(p), _bits(p_want))


def test_first_update_copies_bit_for_bit():
    _need_gpu()
    begin, length = 64, 1028
    avg0, p0, inside = _poisoned_pair(begin, length, seed=5)
    special = torch.tensor([0x7FC00001, 0x7F800123, -0x00400000 + 0x7F, 0x7F800000, -0x00800000, 1, 0x007FFFFF, -0x7FFFFFFF,
                            0, -0x80000000], dtype=torch.int64).to(torch.int32)
    # quiet and signalling NaNs with payloads, a negative NaN, +inf, -inf, the smallest and the largest denormal, a negative
    # denormal, +0 and -0: across the end of the first tile and in the last float4
    pv = p0.view(torch.int32)
    pv[begin + 1020:begin + 1020 + special.numel() - 2] = special[:-2]
    pv[begin + length - 2:begin + length] = special[-2:]
    pv[begin:begin + 4] = special[:4]
    for kind in KINDS:
        avg, p = avg0.cuda(), p0.cuda()
        n, ticket = _state(0)
        _launch(avg, p, begin, begin + length, KINDS[kind], 1.0 - DECAY, n, ticket)
        assert int(n) == 1 and int(ticket) == 0
        assert torch.equal(_bits(avg)[inside], _bits(p0)[inside])
        assert torch.equal(_bits(avg)[~inside], _bits(avg0)[~inside])
        assert torch.equal(_bits(p), _bits(p0))


@pytest.mark.parametrize("length", [TILE, FULL_GRID], ids=["one_workgroup", "full_grid"])
def test_ticket_advances_the_count_once_per_launch(length):
    _need_gpu()
    avg0, p0, inside = _poisoned_pair(0, length, seed=6)
    runs = []
    for _ in range(2):
        avg, p = avg0.cuda(), p0.cuda()
        n, ticket = _state(0)
        for i in range(1, 6):
            _launch(avg, p, 0, length, _lib.MFM_AVG_SWA, 0.0, n, ticket)
            assert int(n) == i and int(ticket) == 0
            p[:length] += 0.25
        runs.append(_bits(avg))
    assert torch.equal(runs[0], runs[1])
    assert not torch.equal(runs[0][inside], _bits(p0)[inside])


def test_launch_replays_from_a_captured_graph():
    _need_gpu()
    begin, length = 64, 3 * 1024 + 4
    avg0, p0, inside = _poisoned_pair(begin, length, seed=7)
    for kind in KINDS:
        eager, p = avg0.cuda(), p0.cuda()
        n_e, t_e = _state(0)
        for _ in range(3):
            _launch(eager, p, begin, begin + length, KINDS[kind], 1.0 - DECAY, n_e, t_e)
            p[begin:begin + length] += 0.5
        avg, p = avg0.cuda(), p0.cuda()                # static buffers of the graph (the code object is loaded by now)
        n, ticket = _state(0)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _launch(avg, p, begin, begin + length, KINDS[kind], 1.0 - DECAY, n, ticket)
        assert int(n) == 0 and torch.equal(_bits(avg), _bits(avg0))         # (captured, not run)
        for _ in range(3):
            graph.replay()
            p[begin:begin + length] += 0.5
        torch.cuda.synchronize()
        assert int(n) == 3 and int(ticket) == 0
        assert torch.equal(_bits(avg), _bits(eager))
        assert not torch.equal(_bits(avg)[inside], _bits(p0)[inside])


# ----------------------------------------------------------------------------------- the reference loop
B, T_STEPS = 5, 7


def _setup(cls="MFM_KL_EF", seed=7):
    cfgs = configs.canonical_configs(dropout=False)
    model = _model(cfgs, cls=cls)
    optimizer = optim.Adam(model.parameters())                     # before .to(device), as in the reference
    model = model.to("cuda")
    xn, yn = synth.make_batch(cfgs[0]["input_dims"], B, T_STEPS, seed=seed)
    return model, optimizer, torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda(), cfgs[0]


def _step(model, optimizer, X, y, cfg):
    _reference_loop(model, optimizer, X, y, cfg, 1)


def _flat_only(monkeypatch):
    """torch's update raises: whatever runs under this took the flat path"""
    def refuse(self, model):
        raise AssertionError("torch's AveragedModel.update_parameters was called: not the flat path")
    monkeypatch.setattr(T.AveragedModel, "update_parameters", refuse)


def _spy(monkeypatch):
    real, calls = T.AveragedModel.update_parameters, []

    def counting(self, model):
        calls.append(type(self))
        return real(self, model)
    monkeypatch.setattr(T.AveragedModel, "update_parameters", counting)
    return calls


def _assert_close_to_twin(ours, twin, source, k, what):
    """every averaged tensor within k * 2^-21 * max(|avg|, |p|) of torch's twin, the counts equal"""
    assert int(ours.n_averaged) == int(twin.n_averaged), what
    worst = 0.0
    for (name, a), b, p in zip(ours.module.named_parameters(), twin.module.parameters(), source.parameters()):
        bound = max(k, 1) * ULP_BOUND * max(float(b.abs().max()), float(p.abs().max()), 1e-30)
        err = float((a.detach() - b.detach()).abs().max()) if a.numel() else 0.0
        worst = max(worst, err / bound)
        assert err < bound and (k > 0 or err == 0.0), (what, name, err, bound)          # (k == 0: the first update is a copy)
    return worst


def _eval_outputs(avg_model, X):
    avg_model.eval()
    with torch.no_grad():
        decoded, _, _ = avg_model(X)
    return [d.detach().cpu().numpy() for d in decoded]


def _training_state(model, optimizer):
    """everything the next training step reads: the flat parameter and gradient buffers (padding and guard granule included),
    the optimizer's flat moments and step counts, the model's gradient bookkeeping"""
    st = optimizer._fused[model]
    tensors = [_bits(t) for t in (model.engine.params, model._grad_flat, st["m"], st["v"])]
    book = (st["steps"].copy(), model._grad_fresh, model._grad_present.copy(), model._handover_ok(), model._fast_last,
            model._grad_views_attached(), optimizer._fallback is None, [g["lr"] for g in optimizer.param_groups])
    return tensors, book


def _assert_same_state(a, b, what):
    assert len(a[0]) == len(b[0]), what
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y), what
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y), what


def _averaging_run(cls, steps, monkeypatch):
    """The unchanged loop with an EMA and an SWA averager updated after every step, ours on the flat path and torch's on twins.

    That the feature changes no training behaviour is checked where it can be checked exactly: everything the next step reads
    -- parameters, gradients, optimizer state, bookkeeping -- is bit-identical before and after the updates of every step.  (Two
    separate training runs are no yardstick for that: the step's weight- and bias-gradient sums use float atomics, whose
    order, and with it the last bits of a trajectory, may differ from run to run with or without any averaging.)"""
    model, optimizer, X, y, cfg = _setup(cls)
    _step(model, optimizer, X, y, cfg)                  # (the source is on its engine from its first forward on)
    ours = {"ema": S.AveragedModel(model, multi_avg_fn=S.get_ema_multi_avg_fn(DECAY)), "swa": S.AveragedModel(model)}
    twin = {"ema": T.AveragedModel(model, multi_avg_fn=T.get_ema_multi_avg_fn(DECAY)), "swa": T.AveragedModel(model)}
    real = T.AveragedModel.update_parameters
    worst = 0.0
    for step in range(steps):
        if step:
            _step(model, optimizer, X, y, cfg)
        before = _training_state(model, optimizer)
        _flat_only(monkeypatch)
        for key in ours:
            ours[key].update_parameters(model)
        monkeypatch.setattr(T.AveragedModel, "update_parameters", real)
        _assert_same_state(before, _training_state(model, optimizer), (cls, step))
        for key in ours:
            twin[key].update_parameters(model)
            worst = max(worst, _assert_close_to_twin(ours[key], twin[key], model, step, (cls, key, step)))
    cases.report("swa_model_rel_to_bound_%s" % cls, worst)
    print("swa_model_rel_to_bound_%s %.3e" % (cls, worst))
    for key in ours:
        assert ours[key].module._flat_ok() and ours[key].module._engine is not model._engine
        got, want = _eval_outputs(ours[key], X), _eval_outputs(twin[key], X)
        for g, w in zip(got, want):
            assert cases.rel_err(g, w) < 1e-5, (cls, key, cases.rel_err(g, w))
    assert model._handover_ok() and optimizer._fallback is None and model._grad_views_attached()
    assert model.training                                # (the averaged copies went to eval mode, the source did not)


def test_unchanged_loop_with_both_averagers_follows_torchs_twins_and_leaves_training_alone(monkeypatch):
    _need_gpu()
    _averaging_run("MFM_KL_EF", 6, monkeypatch)


def test_mfm_kl_and_its_104_tensors(monkeypatch):
    _need_gpu()
    assert len(_model(configs.canonical_configs(dropout=False), cls="MFM_KL")._plist) == 104
    _averaging_run("MFM_KL", 3, monkeypatch)


def test_flat_path_does_not_synchronise(monkeypatch):
    _need_gpu()
    model, optimizer, X, y, cfg = _setup()
    _step(model, optimizer, X, y, cfg)
    _flat_only(monkeypatch)
    ema = S.AveragedModel(model, multi_avg_fn=S.get_ema_multi_avg_fn(DECAY))
    swa = S.AveragedModel(model, avg_fn=S.get_swa_avg_fn())
    ema.update_parameters(model)                        # (first call: the copy's engine is adopted, the ticket allocated)
    swa.update_parameters(model)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            ema.update_parameters(model)
            swa.update_parameters(model)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(ema.n_averaged) == 3 and int(swa.n_averaged) == 3
    assert ema._mfm_ticket is not swa._mfm_ticket and int(ema._mfm_ticket) == 0 and int(swa._mfm_ticket) == 0


def _plain_twins(make, kw_ours, kw_torch):
    """(source, ours, torch's) for a source module built by make()"""
    src = make()
    return src, S.AveragedModel(src, **kw_ours), T.AveragedModel(src, **kw_torch)


def _nudge(module, k):
    with torch.no_grad():
        for p in module.parameters():
            p.add_(0.01 * (k + 1))


def _assert_fallback_equals_torch(src, ours, twin, calls, updates=3):
    for k in range(updates):
        _nudge(src, k)
        before = len(calls)
        ours.update_parameters(src)
        assert calls[before:] == [S.AveragedModel], "the update did not go to torch's method"
        twin.update_parameters(src)
        assert int(ours.n_averaged) == int(twin.n_averaged) == k + 1
        for a, b in zip(ours.parameters(), twin.parameters()):
            assert torch.equal(a, b)


def test_fallbacks_go_to_torch_and_equal_it_bit_for_bit(monkeypatch):
    _need_gpu()
    from factorized_amd import mfm_extra as X_
    calls = _spy(monkeypatch)
    model, optimizer, X, y, cfg = _setup()
    _step(model, optimizer, X, y, cfg)
    custom = lambda a, p, n: 0.5 * a + 0.5 * p
    # a custom avg_fn; a function from torch's own factory (an opaque closure: not recognised)
    for kw_o, kw_t in ((dict(avg_fn=custom), dict(avg_fn=custom)),
                       (dict(multi_avg_fn=T.get_ema_multi_avg_fn(DECAY)), dict(multi_avg_fn=T.get_ema_multi_avg_fn(DECAY)))):
        _assert_fallback_equals_torch(model, S.AveragedModel(model, **kw_o), T.AveragedModel(model, **kw_t), calls)
    # a composed model of mfm_extra.py; a plain nn.Linear on the GPU -- under a rule the flat path would take
    ema = lambda M: dict(multi_avg_fn=M.get_ema_multi_avg_fn(DECAY))
    torch.manual_seed(3)
    for make in (lambda: X_.M_D(*configs.canonical_configs(dropout=False)).cuda(), lambda: nn.Linear(7, 5).cuda()):
        src, ours, twin = _plain_twins(make, ema(S), ema(T))
        _assert_fallback_equals_torch(src, ours, twin, calls)
    # a source model whose parameters left the flat buffer (a .to() round trip; no forward since)
    model.fast_grads = False
    model.to("cpu")
    model.to("cuda")
    assert not model._flat_ok()
    _assert_fallback_equals_torch(model, S.AveragedModel(model, **ema(S)), T.AveragedModel(model, **ema(T)), calls)


def test_flat_and_torch_updates_alternate_on_one_count(monkeypatch):
    _need_gpu()
    model, optimizer, X, y, cfg = _setup()
    _step(model, optimizer, X, y, cfg)
    ours = S.AveragedModel(model, multi_avg_fn=S.get_ema_multi_avg_fn(DECAY))
    twin = T.AveragedModel(model, multi_avg_fn=T.get_ema_multi_avg_fn(DECAY))
    calls = _spy(monkeypatch)
    for k in range(6):
        _step(model, optimizer, X, y, cfg)
        before = len(calls)
        if k % 2:
            T.AveragedModel.update_parameters(ours, model)          # torch's path on our instance
            assert calls[before:] == [S.AveragedModel]
        else:
            ours.update_parameters(model)                           # the flat path
            assert calls[before:] == []
        twin.update_parameters(model)
        _assert_close_to_twin(ours, twin, model, k, ("alternate", k))
    assert int(ours.n_averaged) == 6


def test_copies_and_checkpoints_continue_the_trajectory(monkeypatch):
    _need_gpu()
    model, optimizer, X, y, cfg = _setup()
    _step(model, optimizer, X, y, cfg)
    make = lambda: S.AveragedModel(model, multi_avg_fn=S.get_ema_multi_avg_fn(DECAY))
    ours = make()
    _flat_only(monkeypatch)
    for _ in range(3):
        _step(model, optimizer, X, y, cfg)
        ours.update_parameters(model)
    sd = ours.state_dict()
    assert set(sd) == {"n_averaged"} | {"module." + n for n in model.state_dict()} and not any("ticket" in k for k in sd)
    clone = copy.deepcopy(ours)
    assert clone._mfm_ticket is None and ours._mfm_ticket is not None
    fresh = make()
    fresh.load_state_dict(copy.deepcopy(sd))
    for _ in range(3):
        _step(model, optimizer, X, y, cfg)
        for a in (ours, clone, fresh):
            a.update_parameters(model)
    assert clone._mfm_ticket is not None and clone._mfm_ticket is not ours._mfm_ticket
    for a in (clone, fresh):
        assert int(a.n_averaged) == int(ours.n_averaged) == 6
        for p, q in zip(a.parameters(), ours.parameters()):
            assert torch.equal(p, q)
    assert not torch.equal(_bits(ours.module.engine.params), _bits(model.engine.params))
