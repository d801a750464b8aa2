"""factorized_amd.swa_utils without a GPU: torch's names, a strict subclass of torch's AveragedModel, the native entry point and
its host-side argument checks, torch's factory error texts, and bit-identical updates on a plain CPU module (the path everything
outside a pair of fused models takes), state dicts included."""
import copy
import ctypes as C

import pytest
import torch
import torch.nn as nn
import torch.optim.swa_utils as T

import factorized_amd.optim as optim
from factorized_amd import _lib, swa_utils as S


def test_module_exports_torchs_names_and_is_reachable_from_optim():
    assert sorted(S.__all__) == sorted(T.__all__)
    for name in T.__all__:
        assert hasattr(S, name), name
    assert optim.swa_utils is S
    assert S.SWALR is T.SWALR and S.update_bn is T.update_bn


def test_averaged_model_is_a_strict_subclass():
    assert S.AveragedModel is not T.AveragedModel and issubclass(S.AveragedModel, T.AveragedModel)
    a = S.AveragedModel(nn.Linear(3, 2))
    assert isinstance(a, T.AveragedModel)
    import inspect
    assert list(inspect.signature(S.AveragedModel.__init__).parameters) == list(inspect.signature(T.AveragedModel.__init__).parameters)
    with pytest.raises(AssertionError, match="Only one of avg_fn and multi_avg_fn"):
        S.AveragedModel(nn.Linear(3, 2), avg_fn=S.get_swa_avg_fn(), multi_avg_fn=S.get_swa_multi_avg_fn())


def test_library_exports_the_entry_point():
    L = _lib.lib()
    assert hasattr(L, "mfm_avg_flat") and "mfm_avg_flat" in _lib.exported_names()
    assert (_lib.MFM_AVG_SWA, _lib.MFM_AVG_EMA) == (0, 1)
    assert L.mfm_abi_version() == 5


def test_avg_launch_validates_on_the_host():
    """argument errors are caught before anything is enqueued (no device memory is touched: the pointers are never used)"""
    L = _lib.lib()
    fake = C.c_void_p(1 << 20)                    # 16-byte aligned, never dereferenced: every call below is refused first
    nan = float("nan")
    cases = [
        (dict(avg=None), b"must not be null"),
        (dict(p=None), b"must not be null"),
        (dict(n=None), b"must not be null"),
        (dict(ticket=None), b"must not be null"),
        (dict(avg=C.c_void_p((1 << 20) + 4)), b"16-byte aligned"),
        (dict(p=C.c_void_p((1 << 20) + 8)), b"16-byte aligned"),
        (dict(begin=2), b"multiples of 4"),
        (dict(end=1022), b"multiples of 4"),
        (dict(begin=64, end=64), b"end above begin"),
        (dict(begin=128, end=64), b"end above begin"),
        (dict(kind=2), b"unknown kind"),
        (dict(kind=-1), b"unknown kind"),
        (dict(kind=_lib.MFM_AVG_EMA, w=-0.1), b"EMA weight"),
        (dict(kind=_lib.MFM_AVG_EMA, w=1.5), b"EMA weight"),
        (dict(kind=_lib.MFM_AVG_EMA, w=nan), b"EMA weight"),
        (dict(n=C.c_void_p((1 << 20) + 4)), b"8-byte aligned"),
    ]
    for over, msg in cases:
        rc = L.mfm_avg_flat(over.get("avg", fake), over.get("p", fake), over.get("begin", 0), over.get("end", 1024),
                            over.get("kind", _lib.MFM_AVG_SWA), over.get("w", 0.1), over.get("n", fake), over.get("ticket", fake),
                            None)
        assert rc == -1, over
        assert msg in L.mfm_last_error(), (over, L.mfm_last_error())


@pytest.mark.parametrize("factory", ["get_ema_multi_avg_fn", "get_ema_avg_fn"])
@pytest.mark.parametrize("decay", [-0.1, 1.1])
def test_factories_raise_torchs_error_text(factory, decay):
    with pytest.raises(ValueError) as ours:
        getattr(S, factory)(decay)
    with pytest.raises(ValueError) as theirs:
        getattr(T, factory)(decay)
    assert str(ours.value) == str(theirs.value) and "Invalid decay value" in str(ours.value)


def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(5, 7), nn.Tanh(), nn.Linear(7, 3))


RULES = {
    "default": lambda M: {},
    "ema_multi": lambda M: dict(multi_avg_fn=M.get_ema_multi_avg_fn(0.9)),
    "swa_multi": lambda M: dict(multi_avg_fn=M.get_swa_multi_avg_fn()),
    "ema": lambda M: dict(avg_fn=M.get_ema_avg_fn(0.9)),
    "swa": lambda M: dict(avg_fn=M.get_swa_avg_fn()),
}


def _walk(net, step):
    """the parameters move: what an optimizer step would do between two updates"""
    with torch.no_grad():
        for k, p in enumerate(net.parameters()):
            p.add_(0.01 * (step + 1) * torch.cos(torch.arange(p.numel(), dtype=torch.float32) + k).view_as(p))


@pytest.mark.parametrize("rule", list(RULES))
def test_cpu_updates_bit_identical_to_torch(rule):
    net = _net()
    ours, ref = S.AveragedModel(net, **RULES[rule](S)), T.AveragedModel(net, **RULES[rule](T))
    for step in range(5):
        _walk(net, step)
        ours.update_parameters(net)
        ref.update_parameters(net)
        assert torch.equal(ours.n_averaged, ref.n_averaged) and int(ours.n_averaged) == step + 1
        for p, q in zip(ours.parameters(), ref.parameters()):
            assert torch.equal(p, q), (rule, step)
    assert not torch.equal(next(ours.parameters()), next(net.parameters()))        # (an average, not the last copy)
    x = torch.randn(4, 5)
    assert torch.equal(ours(x), ref(x))


def test_state_dicts_have_the_same_keys_and_load_both_ways():
    net = _net()
    ours = S.AveragedModel(net, multi_avg_fn=S.get_ema_multi_avg_fn(0.9))
    ref = T.AveragedModel(net, multi_avg_fn=T.get_ema_multi_avg_fn(0.9))
    for step in range(3):
        _walk(net, step)
        ours.update_parameters(net)
        ref.update_parameters(net)
    assert set(ours.state_dict()) == set(ref.state_dict())
    assert "n_averaged" in ours.state_dict() and all(k == "n_averaged" or k.startswith("module.") for k in ours.state_dict())
    fresh_ours, fresh_ref = S.AveragedModel(_net()), T.AveragedModel(_net())
    fresh_ours.load_state_dict(copy.deepcopy(ref.state_dict()))            # torch's -> ours
    fresh_ref.load_state_dict(copy.deepcopy(ours.state_dict()))            # ours -> torch's
    for a in (fresh_ours, fresh_ref):
        assert int(a.n_averaged) == 3
        for p, q in zip(a.parameters(), ref.parameters()):
            assert torch.equal(p, q)


def test_deepcopy_and_pickle_drop_the_ticket_word():
    import io
    a = S.AveragedModel(_net())
    a._mfm_ticket = torch.zeros(1, dtype=torch.int32)
    b = copy.deepcopy(a)
    assert b._mfm_ticket is None and a._mfm_ticket is not None
    buf = io.BytesIO()
    torch.save(a, buf)
    buf.seek(0)
    c = torch.load(buf, weights_only=False)
    assert c._mfm_ticket is None and isinstance(c, S.AveragedModel)
    assert "_mfm_ticket" not in a.state_dict()
