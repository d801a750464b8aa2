"""factorized_amd.optim.Adam / AdamW without a GPU: torch.optim.Adam's whole signature and constructor checks, the native entry
points of the span kernel with every option (host-side validation only), and bit-identical steps on plain CPU modules (the
path every parameter outside a fused model takes)."""
import copy
import ctypes as C
import inspect

import pytest
import torch
import torch.nn as nn

import factorized_amd.optim as optim
from factorized_amd import _lib


def test_adamw_is_its_own_optimizer_class_and_adam_takes_every_keyword():
    assert optim.AdamW is not torch.optim.AdamW and optim.Adam is not torch.optim.Adam
    assert issubclass(optim.AdamW, optim.Adam) and issubclass(optim.Adam, torch.optim.Optimizer)
    assert not issubclass(optim.Adam, torch.optim.Adam)
    for ours, theirs in ((optim.Adam, torch.optim.Adam), (optim.AdamW, torch.optim.AdamW)):
        a, b = inspect.signature(ours.__init__).parameters, inspect.signature(theirs.__init__).parameters
        assert set(a) == set(b)
        for k in b:
            assert a[k].default == b[k].default and a[k].kind == b[k].kind, (ours.__name__, k)
    g = optim.AdamW(nn.Linear(3, 2).parameters()).param_groups[0]
    assert g["weight_decay"] == 1e-2 and g["decoupled_weight_decay"] is True
    g = optim.Adam(nn.Linear(3, 2).parameters(), weight_decay=1e-5, amsgrad=True, maximize=True, foreach=None,
                   decoupled_weight_decay=False, capturable=False, differentiable=False, fused=None).param_groups[0]
    assert (g["weight_decay"], g["amsgrad"], g["maximize"], g["decoupled_weight_decay"]) == (1e-5, True, True, False)


def test_library_exports_the_adam_ext_entry_points():
    L = _lib.lib()
    for name in ("mfm_adam_ext_flat_spans", "mfm_adam_ext_flat_spans_guarded"):
        assert hasattr(L, name) and name in _lib.exported_names()
    assert C.sizeof(_lib.AdamExtSpan) == 48
    # a span table is a kernel argument (4 KiB): not every tensor of MFM_KL (104) fits, two launches do
    assert 52 <= _lib.MFM_ADAMX_MAX_SPANS < 104


def _span(**over):
    a = (_lib.AdamExtSpan * 1)()
    a[0].begin, a[0].end, a[0].step, a[0].flags = over.get("begin", 0), over.get("end", 64), over.get("step", 1), over.get("flags", 0)
    a[0].lr, a[0].beta1, a[0].beta2 = over.get("lr", 1e-3), over.get("beta1", 0.9), over.get("beta2", 0.999)
    a[0].eps, a[0].weight_decay = over.get("eps", 1e-8), over.get("weight_decay", 0.0)
    return a


def test_adam_ext_launch_validates_on_the_host():
    """argument errors are caught before anything is enqueued (no device memory is touched: the pointers are never used)"""
    L = _lib.lib()
    fake = C.c_void_p(1 << 20)                    # 16-byte aligned, never dereferenced: every call below is refused first
    cases = [
        (dict(p=None), b"bad arguments"),
        (dict(v=None), b"bad arguments"),
        (dict(n=0), b"bad arguments"),
        (dict(n=_lib.MFM_ADAMX_MAX_SPANS + 1), b"at most"),
        (dict(g=C.c_void_p((1 << 20) + 4)), b"16-byte aligned"),
        (dict(vmax=C.c_void_p((1 << 20) + 8)), b"16-byte aligned"),
        (dict(begin=2), b"multiples of 4"),
        (dict(end=62), b"multiples of 4"),
        (dict(end=0), b"multiples of 4"),
        (dict(step=0), b"step 0"),
        (dict(lr=-1.0), b">= 0"),
        (dict(eps=-1e-8), b">= 0"),
        (dict(weight_decay=-1e-2), b">= 0"),
        (dict(beta1=1.0), b"[0, 1)"),
        (dict(beta2=1.5), b"[0, 1)"),
        (dict(beta1=-0.1), b"[0, 1)"),
        (dict(flags=64), b"unknown flags"),
        (dict(flags=_lib.MFM_ADAMX_AMSGRAD, vmax=None), b"vmax"),
    ]
    for over, msg in cases:
        for guarded in (False, True):
            args = [over.get("p", fake), over.get("g", fake), over.get("m", fake), over.get("v", fake), over.get("vmax", fake),
                    _span(**over), over.get("n", 1), 1.0]
            if guarded:
                rc = L.mfm_adam_ext_flat_spans_guarded(*args, fake, None)
            else:
                rc = L.mfm_adam_ext_flat_spans(*args, None)
            assert rc == -1, over
            assert msg in L.mfm_last_error(), (over, L.mfm_last_error())
    two = (_lib.AdamExtSpan * 2)()
    for k, (b, e) in enumerate(((0, 128), (64, 192))):            # overlapping
        two[k].begin, two[k].end, two[k].step, two[k].lr, two[k].beta1, two[k].beta2 = b, e, 1, 1e-3, 0.9, 0.999
    assert L.mfm_adam_ext_flat_spans(fake, fake, fake, fake, None, two, 2, 1.0, None) == -1
    assert b"disjoint" in L.mfm_last_error()
    two[0].begin, two[0].end, two[1].begin, two[1].end = 64, 128, 0, 64          # not ascending
    assert L.mfm_adam_ext_flat_spans(fake, fake, fake, fake, None, two, 2, 1.0, None) == -1
    assert b"ascending" in L.mfm_last_error()


def test_adam_flat_spans_validates_on_the_host():
    """mfm_adam_flat_spans takes its spans in any order: its refusals come before anything is enqueued (the pointers are never
    used)"""
    L = _lib.lib()
    fake = C.c_void_p(1 << 20)

    def call(spans, n=None, guarded=False):
        arr = (_lib.AdamSpan * len(spans))()
        for a, (b, e, st) in zip(arr, spans):
            a.begin, a.end, a.step = b, e, st
        args = [fake, fake, fake, fake, arr, len(spans) if n is None else n, 1e-3, 0.9, 0.999, 1e-8, 1.0]
        if guarded:
            return L.mfm_adam_flat_spans_guarded(*args, fake, None)
        return L.mfm_adam_flat_spans(*args, None)

    nine = [(64 * k, 64 * k + 64, 1) for k in range(_lib.MFM_ADAM_MAX_SPANS + 1)]
    cases = [
        ([(0, 128, 1), (64, 192, 1)], b"overlaps spans[0]"),
        ([(64, 192, 2), (0, 128, 1)], b"overlaps spans[0]"),     # descending
        ([(0, 64, 1), (256, 320, 1), (128, 260, 1)], b"spans[2]: [128,260) overlaps spans[1]"),
        (nine, b"nspans=9"),
        ([(2, 64, 1)], b"multiples of 4"),
        ([(0, 62, 1)], b"multiples of 4"),
        ([(0, 64, 1), (64, 130, 1)], b"multiples of 4"),
        ([(0, 64, 0)], b"step 0"),
        ([(0, 64, 1), (128, 192, 0)], b"step 0"),
    ]
    for spans, msg in cases:
        for guarded in (False, True):
            assert call(spans, guarded=guarded) != 0, spans
            assert msg in L.mfm_last_error(), (spans, L.mfm_last_error())
    assert call([(0, 64, 1)], n=0) != 0 and b"bad arguments" in L.mfm_last_error()


CTOR_CASES = [
    dict(lr=-0.1),
    dict(eps=-1e-8),
    dict(betas=(1.0, 0.999)),
    dict(betas=(0.9, 1.0)),
    dict(betas=(-0.1, 0.999)),
    dict(weight_decay=-1e-4),
    dict(betas=(0.9, torch.tensor(0.999))),
    dict(betas=(torch.tensor([0.9, 0.8]), torch.tensor(0.999))),
    dict(betas=(torch.tensor(0.9), torch.tensor([0.9, 0.99]))),
    dict(lr=torch.tensor([0.1, 0.2])),
    dict(lr=torch.tensor(0.1), foreach=True),
    dict(betas=(torch.tensor(0.9), torch.tensor(0.99)), foreach=True),
    dict(betas=(torch.tensor(0.8), torch.tensor(0.99))),
    dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=1e-3, amsgrad=True, maximize=True),
    dict(weight_decay=1e-2, decoupled_weight_decay=True, foreach=False),
    dict(),
]
_KEYS = ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused",
         "decoupled_weight_decay")


@pytest.mark.parametrize("cls", ["Adam", "AdamW"])
@pytest.mark.parametrize("kw", CTOR_CASES, ids=[str(sorted(k.keys())) + str(i) for i, k in enumerate(CTOR_CASES)])
def test_constructor_validation_matches_torch(cls, kw):
    if cls == "AdamW" and "decoupled_weight_decay" in kw:
        kw = {k: v for k, v in kw.items() if k != "decoupled_weight_decay"}          # (not a keyword of AdamW, in torch either)

    def outcome(c):
        try:
            opt = c(nn.Linear(3, 2).parameters(), **kw)
        except Exception as e:          # noqa: BLE001 -- the exception class and text are what is compared
            return type(e), str(e)
        g = opt.param_groups[0]
        return {k: g[k] for k in _KEYS}
    assert outcome(getattr(optim, cls)) == outcome(getattr(torch.optim, cls))


def test_adamw_refuses_the_decay_style_keyword_like_torch():
    for c in (optim.AdamW, torch.optim.AdamW):
        with pytest.raises(TypeError):
            c(nn.Linear(3, 2).parameters(), decoupled_weight_decay=False)


def test_constructor_rejects_differentiable_and_fused():
    for cls in (optim.Adam, optim.AdamW):
        for kw in (dict(differentiable=True), dict(fused=True)):
            with pytest.raises(ValueError, match="factorized_amd.optim." + cls.__name__):
                cls(nn.Linear(3, 2).parameters(), **kw)


def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(5, 7), nn.Tanh(), nn.Linear(7, 3), nn.Tanh(), nn.Linear(3, 1))


STEP_CASES = {
    "plain": ("Adam", dict(lr=0.01)),
    "l2": ("Adam", dict(lr=0.01, weight_decay=1e-2)),
    "decoupled": ("Adam", dict(lr=0.01, weight_decay=1e-2, decoupled_weight_decay=True)),
    "amsgrad": ("Adam", dict(lr=0.01, amsgrad=True)),
    "maximize": ("Adam", dict(lr=0.01, maximize=True)),
    "amsgrad_l2_maximize": ("Adam", dict(lr=0.02, betas=(0.8, 0.99), eps=1e-6, weight_decay=3e-3, amsgrad=True, maximize=True)),
    "adamw": ("AdamW", dict(lr=0.01)),
    "adamw_amsgrad_maximize": ("AdamW", dict(lr=0.01, weight_decay=0.1, amsgrad=True, maximize=True)),
}


def _groups(net, two_groups):
    if not two_groups:
        return [dict(params=list(net.parameters()))]
    return [dict(params=list(net[0].parameters()) + list(net[4].parameters())),
            dict(params=list(net[2].parameters()), lr=0.003, betas=(0.5, 0.9), weight_decay=0.05, amsgrad=False)]


def _step_all(pairs, x, step):
    zero_kw = {"set_to_none": False} if step % 2 else {}
    for net, opt in pairs:
        opt.zero_grad(**zero_kw)
        out = net(x + 0.1 * step)
        loss = (out ** 2).mean() if step != 3 else out.abs().mean()
        loss.backward()
        opt.step()


@pytest.mark.parametrize("two_groups", [False, True])
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_cpu_steps_bit_identical_to_torch(name, two_groups):
    """several steps on a plain CPU module: the same bits as torch.optim.Adam / AdamW -- including a parameter that never gets a
    gradient (skipped, no state, no decoupled decay) and the PyTorch-0.4 zero_grad(set_to_none=False) pattern"""
    cls, kw = STEP_CASES[name]
    a = _net()
    extra = nn.Parameter(torch.randn(4))                      # in the optimizer, never in the loss: .grad stays None
    b = copy.deepcopy(a)
    extra_b = nn.Parameter(extra.detach().clone())
    ga, gb = _groups(a, two_groups), _groups(b, two_groups)
    ga[0]["params"].append(extra)
    gb[0]["params"].append(extra_b)
    ours, ref = getattr(optim, cls)(ga, **kw), getattr(torch.optim, cls)(gb, **kw)
    torch.manual_seed(1)
    x = torch.randn(16, 5)
    for step in range(6):
        _step_all(((a, ours), (b, ref)), x, step)
        for p, q in zip(list(a.parameters()) + [extra], list(b.parameters()) + [extra_b]):
            assert torch.equal(p, q), (name, step)
    assert extra.grad is None and torch.equal(extra, extra_b) and extra not in ours._fallback.state
    for p, q in zip(a.parameters(), b.parameters()):
        s, r = ours._fallback.state[p], ref.state[q]
        assert set(s) == set(r)
        for k in r:
            assert torch.equal(s[k], r[k]), (name, k)


def test_cpu_reduce_lr_on_plateau_acts_on_the_outer_groups():
    a = _net()
    b = copy.deepcopy(a)
    ours, ref = optim.AdamW(a.parameters(), lr=0.01), torch.optim.AdamW(b.parameters(), lr=0.01)
    sa = optim.ReduceLROnPlateau(ours, "min", patience=0, factor=0.1)
    sb = torch.optim.lr_scheduler.ReduceLROnPlateau(ref, "min", patience=0, factor=0.1)
    x = torch.randn(8, 5)
    for k in range(5):
        _step_all(((a, ours), (b, ref)), x, 0)
        sa.step(1.0 + k)
        sb.step(1.0 + k)                     # no improvement: the rate drops
    assert ours.param_groups[0]["lr"] == ref.param_groups[0]["lr"] < 0.01
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)


@pytest.mark.parametrize("name", ["amsgrad_l2_maximize", "adamw"])
def test_cpu_state_dict_round_trip_continues_identically(name):
    cls, kw = STEP_CASES[name]
    a = _net()
    x = torch.randn(8, 5)
    opt = getattr(optim, cls)(a.parameters(), **kw)
    for s in range(3):
        _step_all(((a, opt),), x, s)
    sd = copy.deepcopy(opt.state_dict())
    if kw.get("amsgrad"):
        assert all("max_exp_avg_sq" in s for s in sd["fallback"]["state"].values())
    b = copy.deepcopy(a)
    opt_b = getattr(optim, cls)(b.parameters(), **kw)
    opt_b.load_state_dict(sd)
    for s in range(3):
        _step_all(((a, opt), (b, opt_b)), x, s)
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)


def test_state_saved_before_the_options_existed_still_loads():
    """a checkpoint whose parameter groups carry only lr / betas / eps / weight_decay / amsgrad (what this class saved before it
    took the other keywords) loads, and the missing keys take their defaults"""
    a = _net()
    opt = optim.Adam(a.parameters())
    sd = opt.state_dict()
    for g in sd["param_groups"]:
        for k in ("maximize", "foreach", "capturable", "differentiable", "fused", "decoupled_weight_decay"):
            del g[k]
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert g["maximize"] is False and g["decoupled_weight_decay"] is False and g["foreach"] is None
    _step_all(((a, opt),), torch.randn(8, 5), 0)
