"""factorized_amd.nn_utils without a GPU: the native entry points behind it and their host-side argument checks, and the path
every call takes that is not about ONE fused model on the GPU -- torch's own functions, bit for bit."""
import ctypes as C
import math

import pytest
import torch
import torch.nn as nn

from factorized_amd import _lib, configs, nn_utils


def test_library_exports_the_clip_entry_points():
    L = _lib.lib()
    for name in ("mfm_clip_workspace_floats", "mfm_clip_grad_norm_flat_spans", "mfm_clip_grad_value_flat_spans"):
        assert hasattr(L, name) and name in _lib.exported_names()
    assert C.sizeof(_lib.ClipSpan) == 16
    assert _lib.MFM_CLIP_MAX_SPANS >= 104         # every tensor of the largest fused model (MFM_KL) as its own span
    assert (_lib.MFM_NORM_L2, _lib.MFM_NORM_INF, _lib.MFM_NORM_L1) == (0, 1, 2)
    assert L.mfm_clip_workspace_floats() > 0


def _span(begin=0, end=64):
    a = (_lib.ClipSpan * 1)()
    a[0].begin, a[0].end = begin, end
    return a


def test_clip_launches_validate_on_the_host():
    """argument errors are caught before anything is enqueued (no device memory is touched: the pointers are never used)"""
    L = _lib.lib()
    fake = C.c_void_p(1 << 20)                    # 16-byte aligned, never dereferenced: every call below is refused first
    nan = float("nan")
    norm_cases = [
        (dict(g=None), b"bad arguments"),
        (dict(spans=None), b"bad arguments"),
        (dict(ws=None), b"bad arguments"),
        (dict(total=None), b"bad arguments"),
        (dict(n=0), b"bad arguments"),
        (dict(n=_lib.MFM_CLIP_MAX_SPANS + 1), b"bad arguments"),
        (dict(g=C.c_void_p((1 << 20) + 4)), b"16-byte aligned"),
        (dict(begin=2), b"multiple of 4"),
        (dict(end=0), b"ascending"),
        (dict(kind=3), b"unknown norm_kind"),
        (dict(kind=-1), b"unknown norm_kind"),
        (dict(max_norm=-1.0), b"max_norm"),
        (dict(max_norm=nan), b"max_norm"),
    ]
    for over, msg in norm_cases:
        spans = over["spans"] if "spans" in over else _span(over.get("begin", 0), over.get("end", 64))
        rc = L.mfm_clip_grad_norm_flat_spans(over.get("g", fake), spans, over.get("n", 1), over.get("kind", _lib.MFM_NORM_L2),
                                             over.get("max_norm", 1.0), over.get("ws", fake), over.get("total", fake), None, None)
        assert rc == -1, over
        assert msg in L.mfm_last_error(), (over, L.mfm_last_error())
    value_cases = [
        (dict(g=None), b"bad arguments"),
        (dict(spans=None), b"bad arguments"),
        (dict(n=0), b"bad arguments"),
        (dict(n=_lib.MFM_CLIP_MAX_SPANS + 1), b"bad arguments"),
        (dict(g=C.c_void_p((1 << 20) + 8)), b"16-byte aligned"),
        (dict(begin=6), b"multiple of 4"),
        (dict(clip=-0.5), b"clip_value"),
        (dict(clip=nan), b"clip_value"),
    ]
    for over, msg in value_cases:
        spans = over["spans"] if "spans" in over else _span(over.get("begin", 0), over.get("end", 64))
        rc = L.mfm_clip_grad_value_flat_spans(over.get("g", fake), spans, over.get("n", 1), over.get("clip", 1.0), None, None)
        assert rc == -1, over
        assert msg in L.mfm_last_error(), (over, L.mfm_last_error())
    # unordered, and overlapping by one element (an end is any element index: the next begin may not lie below it)
    for b0, e0, b1, e1 in ((64, 128, 0, 64), (0, 65, 64, 128)):
        two = (_lib.ClipSpan * 2)()
        two[0].begin, two[0].end, two[1].begin, two[1].end = b0, e0, b1, e1
        assert L.mfm_clip_grad_norm_flat_spans(fake, two, 2, _lib.MFM_NORM_L2, 1.0, fake, fake, None, None) == -1
        assert b"ascending" in L.mfm_last_error()
        assert L.mfm_clip_grad_value_flat_spans(fake, two, 2, 1.0, None, None) == -1
        assert b"ascending" in L.mfm_last_error()


def _linear_pair():
    torch.manual_seed(0)
    a, b = nn.Linear(7, 5), nn.Linear(7, 5)
    b.load_state_dict(a.state_dict())
    x = torch.randn(9, 7)
    for net in (a, b):
        (net(x) ** 2).sum().backward()
    return a, b


def _klef_pair():
    """two CPU MFM_KL_EF that never saw a GPU, with the same made-up gradients (one tensor left without any)"""
    from factorized_amd import mfm_model as M
    cfgs = configs.canonical_configs(dropout=False)
    a, b = M.MFM_KL_EF(*cfgs), M.MFM_KL_EF(*cfgs)
    gen = torch.Generator().manual_seed(1)
    for k, (p, q) in enumerate(zip(a.parameters(), b.parameters())):
        if k == 3:
            continue
        p.grad = torch.randn(p.shape, generator=gen) * (1.0 + k % 5)
        q.grad = p.grad.clone()
    return a, b


@pytest.mark.parametrize("make", [_linear_pair, _klef_pair], ids=["linear", "klef_cpu"])
@pytest.mark.parametrize("norm_type", [2.0, math.inf, 1.0, 3.0])
@pytest.mark.parametrize("scale", [0.5, 2.0])
def test_cpu_clip_grad_norm_is_torch_bit_for_bit(make, norm_type, scale):
    a, b = make()
    true = float(torch.nn.utils.clip_grad_norm_(list(b.parameters()), math.inf, norm_type))      # (inf: nothing is scaled)
    ours = nn_utils.clip_grad_norm_(a.parameters(), scale * true, norm_type)
    ref = torch.nn.utils.clip_grad_norm_(b.parameters(), scale * true, norm_type)
    assert ours.dim() == 0 and ours.device == ref.device and torch.equal(ours, ref)
    for p, q in zip(a.parameters(), b.parameters()):
        assert (p.grad is None) == (q.grad is None)
        assert p.grad is None or torch.equal(p.grad, q.grad)


@pytest.mark.parametrize("make", [_linear_pair, _klef_pair], ids=["linear", "klef_cpu"])
def test_cpu_clip_grad_value_is_torch_bit_for_bit(make):
    a, b = make()
    assert nn_utils.clip_grad_value_(a.parameters(), 0.05) is None
    torch.nn.utils.clip_grad_value_(b.parameters(), 0.05)
    clipped = 0
    for p, q in zip(a.parameters(), b.parameters()):
        assert (p.grad is None) == (q.grad is None)
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad)
            clipped += int((p.grad.abs() == 0.05).sum())
    assert clipped > 0


def test_cpu_single_tensor_and_empty_list_behave_like_torch():
    a, b = _linear_pair()
    assert torch.equal(nn_utils.clip_grad_norm_(a.weight, 0.1), torch.nn.utils.clip_grad_norm_(b.weight, 0.1))
    assert torch.equal(a.weight.grad, b.weight.grad)
    out = nn_utils.clip_grad_norm_([], 1.0)
    assert out.dim() == 0 and float(out) == 0.0


def test_error_if_nonfinite_raises_torchs_error():
    a, b = _linear_pair()
    for net in (a, b):
        net.weight.grad[0, 0] = float("nan")

    def message(fn, net):
        with pytest.raises(RuntimeError) as e:
            fn(net.parameters(), 1.0, error_if_nonfinite=True)
        return str(e.value)
    ours = message(nn_utils.clip_grad_norm_, a)
    assert ours == message(torch.nn.utils.clip_grad_norm_, b) and "non-finite" in ours
    assert math.isnan(float(nn_utils.clip_grad_norm_(a.parameters(), 1.0)))          # without the flag: a NaN norm, no error
