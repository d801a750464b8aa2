"""factorized_amd.optim.SGD without a GPU: a real torch.optim.Optimizer (not torch's class under another name), the native
entry points it launches, torch.optim.SGD's constructor checks, and bit-identical steps on plain CPU modules (the path every
parameter outside a fused model takes)."""
import copy

import pytest
import torch
import torch.nn as nn

import factorized_amd.optim as optim
from factorized_amd import _lib


def test_sgd_is_its_own_optimizer_class():
    assert optim.SGD is not torch.optim.SGD
    assert issubclass(optim.SGD, torch.optim.Optimizer)
    assert not issubclass(optim.SGD, torch.optim.SGD)


def test_library_exports_the_sgd_entry_points():
    L = _lib.lib()
    for name in ("mfm_sgd_flat_spans", "mfm_sgd_flat_spans_guarded"):
        assert hasattr(L, name) and name in _lib.exported_names()
    assert _lib.MFM_SGD_MAX_SPANS >= 104          # every tensor of the largest fused model (MFM_KL) as its own span
    import ctypes as C
    assert C.sizeof(_lib.SgdSpan) == 40


def test_sgd_launch_validates_on_the_host():
    """argument errors are caught before anything is enqueued (no device memory is touched: the pointers are never used)"""
    import ctypes as C
    L = _lib.lib()
    fake = C.c_void_p(1 << 20)                    # 16-byte aligned, never dereferenced: every call below is refused first
    arr = (_lib.SgdSpan * 1)()
    arr[0].begin, arr[0].end, arr[0].lr, arr[0].momentum = 0, 64, 0.1, 0.9
    cases = [
        (dict(p=None), b"bad arguments"),
        (dict(n=0), b"bad arguments"),
        (dict(n=_lib.MFM_SGD_MAX_SPANS + 1), b"bad arguments"),
        (dict(g=C.c_void_p((1 << 20) + 4)), b"16-byte aligned"),
        (dict(begin=2), b"multiples of 4"),
        (dict(end=0), b"multiples of 4"),
        (dict(lr=-1.0), b">= 0"),
        (dict(flags=64), b"unknown flags"),
        (dict(buf=None), b"momentum buffer"),
    ]
    for over, msg in cases:
        a = (_lib.SgdSpan * 1)()
        a[0].begin, a[0].end = over.get("begin", 0), over.get("end", 64)
        a[0].lr, a[0].momentum, a[0].flags = over.get("lr", 0.1), 0.9, over.get("flags", 0)
        rc = L.mfm_sgd_flat_spans(over.get("p", fake), over.get("g", fake), over.get("buf", fake), a, over.get("n", 1), 1.0, None)
        assert rc == -1, over
        assert msg in L.mfm_last_error(), (over, L.mfm_last_error())
    two = (_lib.SgdSpan * 2)()
    two[0].begin, two[0].end, two[1].begin, two[1].end = 64, 128, 0, 64          # not ascending
    assert L.mfm_sgd_flat_spans(fake, fake, fake, two, 2, 1.0, None) == -1
    assert b"ascending" in L.mfm_last_error()


CTOR_CASES = [
    dict(lr=-0.1),
    dict(lr=0.1, momentum=-0.5),
    dict(lr=0.1, weight_decay=-1e-4),
    dict(lr=0.1, nesterov=True),
    dict(lr=0.1, momentum=0.9, dampening=0.1, nesterov=True),
    dict(lr=torch.tensor([0.1, 0.2])),
    dict(lr=0.1, momentum=0.9, nesterov=True),
    dict(lr=0.1, momentum=0.9, dampening=0.5, weight_decay=1e-3, maximize=True),
    dict(),
]


@pytest.mark.parametrize("kw", CTOR_CASES, ids=[str(sorted(k.keys())) + str(i) for i, k in enumerate(CTOR_CASES)])
def test_constructor_validation_matches_torch(kw):
    def outcome(cls):
        try:
            opt = cls(nn.Linear(3, 2).parameters(), **kw)
        except Exception as e:          # noqa: BLE001 -- the exception class and text are what is compared
            return type(e), str(e)
        g = opt.param_groups[0]
        return {k: g[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize", "foreach")}
    assert outcome(optim.SGD) == outcome(torch.optim.SGD)


def test_constructor_rejects_differentiable_and_fused():
    for kw in (dict(differentiable=True), dict(fused=True)):
        with pytest.raises(ValueError, match="factorized_amd.optim.SGD"):
            optim.SGD(nn.Linear(3, 2).parameters(), lr=0.1, **kw)


def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(5, 7), nn.Tanh(), nn.Linear(7, 3), nn.Tanh(), nn.Linear(3, 1))


STEP_CASES = {
    "plain": dict(lr=0.05),
    "momentum": dict(lr=0.05, momentum=0.9),
    "dampening": dict(lr=0.05, momentum=0.9, dampening=0.3),
    "nesterov": dict(lr=0.05, momentum=0.9, nesterov=True),
    "weight_decay": dict(lr=0.05, momentum=0.9, weight_decay=1e-2),
    "maximize": dict(lr=0.05, momentum=0.5, maximize=True),
    "all": dict(lr=0.02, momentum=0.8, dampening=0.1, weight_decay=3e-3, maximize=True),
}


def _groups(net, kw, two_groups):
    if not two_groups:
        return [dict(params=list(net.parameters()))], kw
    return [dict(params=list(net[0].parameters()) + list(net[4].parameters())),
            dict(params=list(net[2].parameters()), lr=0.01, momentum=0.3, nesterov=False)], kw


@pytest.mark.parametrize("two_groups", [False, True])
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_cpu_steps_bit_identical_to_torch(name, two_groups):
    """several steps on a plain CPU module: the same bits as torch.optim.SGD -- including a parameter that never gets a
    gradient (skipped, no buffer) and the PyTorch-0.4 zero_grad(set_to_none=False) pattern"""
    kw = STEP_CASES[name]
    a = _net()
    extra = nn.Parameter(torch.randn(4))                      # in the optimizer, never in the loss: .grad stays None
    b = copy.deepcopy(a)
    extra_b = nn.Parameter(extra.detach().clone())
    ga, kwa = _groups(a, kw, two_groups)
    gb, kwb = _groups(b, kw, two_groups)
    ga[0]["params"].append(extra)
    gb[0]["params"].append(extra_b)
    ours, ref = optim.SGD(ga, **kwa), torch.optim.SGD(gb, **kwb)
    torch.manual_seed(1)
    x = torch.randn(16, 5)
    for step in range(6):
        zero_kw = {"set_to_none": False} if step % 2 else {}
        for net, opt in ((a, ours), (b, ref)):
            opt.zero_grad(**zero_kw)
            out = net(x + 0.1 * step)
            loss = (out ** 2).mean() if step != 3 else out.abs().mean()
            loss.backward()
            opt.step()
        for p, q in zip(list(a.parameters()) + [extra], list(b.parameters()) + [extra_b]):
            assert torch.equal(p, q), (name, step)
    assert extra.grad is None and torch.equal(extra, extra_b)
    for p, q in zip(a.parameters(), b.parameters()):
        s = ours._fallback.state.get(p, {}).get("momentum_buffer")
        r = ref.state.get(q, {}).get("momentum_buffer")
        assert (s is None) == (r is None) and (s is None or torch.equal(s, r))


def test_cpu_lr_scheduler_acts_on_the_outer_groups():
    a = _net()
    b = copy.deepcopy(a)
    ours, ref = optim.SGD(a.parameters(), lr=0.1, momentum=0.9), torch.optim.SGD(b.parameters(), lr=0.1, momentum=0.9)
    sa = torch.optim.lr_scheduler.StepLR(ours, step_size=2, gamma=0.5)
    sb = torch.optim.lr_scheduler.StepLR(ref, step_size=2, gamma=0.5)
    x = torch.randn(8, 5)
    for _ in range(5):
        for net, opt, sch in ((a, ours, sa), (b, ref, sb)):
            opt.zero_grad()
            net(x).pow(2).mean().backward()
            opt.step()
            sch.step()
    assert ours.param_groups[0]["lr"] == ref.param_groups[0]["lr"] < 0.1
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)


def test_cpu_state_dict_round_trip_continues_identically():
    a = _net()
    x = torch.randn(8, 5)

    def run(net, opt, n):
        for _ in range(n):
            opt.zero_grad()
            net(x).pow(2).mean().backward()
            opt.step()
    opt = optim.SGD(a.parameters(), lr=0.05, momentum=0.9, dampening=0.2)
    run(a, opt, 3)
    sd = copy.deepcopy(opt.state_dict())
    b = copy.deepcopy(a)
    opt_b = optim.SGD(b.parameters(), lr=0.05, momentum=0.9, dampening=0.2)
    opt_b.load_state_dict(sd)
    run(a, opt, 3)
    run(b, opt_b, 3)
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
