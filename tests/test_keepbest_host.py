"""factorized_amd.checkpoint.KeepBest without a GPU: the native entry point and its host-side argument checks, and the torch path
(the one everything outside a fused model on its flat buffer takes) against a twin kept with the reference's own lines,
`if v <= best: best = v; snap = deepcopy(state_dict)` (mfm_mosi.py:467-473): decisions, snapshots bit for bit, restore,
state dicts and copies."""
import copy
import ctypes as C
import io
import os
import re

import pytest
import torch
import torch.nn as nn

from factorized_amd import _lib
from factorized_amd.checkpoint import KeepBest

NAN, INF = float("nan"), float("inf")
METRICS = [3.0, 2.0, 2.0, 5.0, NAN, 1.0, INF]          # improves, improves, ties, worse, NaN, improves, worse
TAKEN = [1, 1, 1, 0, 0, 1, 0]
EPOCHS = [0, 1, 2, 2, 2, 5, 5]
SIGN = {"min": 1.0, "max": -1.0}                        # mode max runs the mirrored sequence


def test_library_exports_the_entry_point_and_the_header_declares_it():
    L = _lib.lib()
    assert hasattr(L, "mfm_keep_best_flat") and "mfm_keep_best_flat" in _lib.exported_names()
    assert (_lib.MFM_KEEP_MIN, _lib.MFM_KEEP_MAX) == (0, 1)
    assert L.mfm_abi_version() == 5                        # (an additive entry: the ABI number stays)
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfm_hip.h")
    text = open(header).read()
    assert re.search(r"\bint\s+mfm_keep_best_flat\s*\(", text)
    assert "typedef struct MfmKeepBestState" in text and "#define MFM_KEEP_MIN 0" in text and "#define MFM_KEEP_MAX 1" in text
    m = re.search(r"typedef struct MfmKeepBestState \{(.*?)\} MfmKeepBestState;", text, re.S)
    fields = re.findall(r"\b(float|int32_t)\s+(\w+)", m.group(1))
    assert fields == [("float", "best_value"), ("int32_t", "calls"), ("int32_t", "best_call"), ("int32_t", "taken"),
                      ("int32_t", "ticket"), ("int32_t", "reserved_")]
    assert _lib.MFM_KEEP_STATE_WORDS == 8


def test_keep_best_launch_validates_on_the_host():
    """argument errors are caught before anything is enqueued (no device memory is touched: the pointers are never used)"""
    L = _lib.lib()
    fake = C.c_void_p(1 << 20)                    # 16-byte aligned, never dereferenced: every call below is refused first
    cases = [
        (dict(best=None), b"must not be null"),
        (dict(p=None), b"must not be null"),
        (dict(state=None), b"must not be null"),
        (dict(best=C.c_void_p((1 << 20) + 4)), b"16-byte aligned"),
        (dict(p=C.c_void_p((1 << 20) + 8)), b"16-byte aligned"),
        (dict(begin=2), b"multiples of 4"),
        (dict(end=1022), b"multiples of 4"),
        (dict(begin=64, end=64), b"end above begin"),
        (dict(begin=128, end=64), b"end above begin"),
        (dict(begin=-4), b"end above begin"),
        (dict(mode=2), b"unknown mode"),
        (dict(mode=-1), b"unknown mode"),
        (dict(state=C.c_void_p((1 << 20) + 4)), b"state must be 16-byte aligned"),
        (dict(state=C.c_void_p((1 << 20) + 8)), b"state must be 16-byte aligned"),
        (dict(metric_dev=C.c_void_p((1 << 20) + 2)), b"device metric 4-byte aligned"),
    ]
    for metric_dev in (None, fake):                # both metric forms
        for over, msg in cases:
            rc = L.mfm_keep_best_flat(over.get("best", fake), over.get("p", fake), over.get("begin", 0), over.get("end", 1024),
                                      over.get("mode", _lib.MFM_KEEP_MIN), over.get("metric_dev", metric_dev), 1.0,
                                      over.get("state", fake), None)
            assert rc == -1, over
            assert msg in L.mfm_last_error(), (over, L.mfm_last_error())


def _net(seed=0):
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Linear(5, 7), nn.BatchNorm1d(7), nn.Tanh(), nn.Linear(7, 3))          # (buffers travel too)
    with torch.no_grad():
        w = net[0].weight.view(-1).view(torch.int32)
        w[0], w[1] = 0x7FC0DEAD, -0x80000000          # a NaN with a payload and -0.0: the snapshot keeps the bits
    return net


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _same(sd_a, sd_b):
    assert list(sd_a) == list(sd_b)
    for k in sd_a:
        assert torch.equal(_bits(sd_a[k]), _bits(sd_b[k])), k


def _walk(net, step):
    """the weights move between two calls, by a plain add_"""
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.01 * (step + 1))


class Twin:
    """the reference's lines, on the host"""

    def __init__(self, net, mode, best):
        self.net, self.mode, self.best, self.snap, self.epoch, self.calls = net, mode, best, None, -1, 0

    def update(self, v):
        take = v <= self.best if self.mode == "min" else v >= self.best
        if take:
            self.best = v
            self.snap = copy.deepcopy(self.net.state_dict())
            self.epoch = self.calls
        self.calls += 1
        return take


def _run(kb, twin, net, metrics, first_step=0):
    taken = []
    for k, v in enumerate(metrics):
        _walk(net, first_step + k)
        took = kb.update(v)
        assert int(took) == int(twin.update(v)), (k, v)
        taken.append(int(took))
        assert kb.last_path == "torch"
        assert kb.calls == twin.calls and kb.epoch == twin.epoch and kb.taken == bool(took)
        assert kb.value == twin.best
        sd = kb.state_dict()
        assert (sd["snapshot"] is None) == (twin.snap is None)
        if twin.snap is not None:
            _same(sd["snapshot"], twin.snap)
    return taken


@pytest.mark.parametrize("mode", ["min", "max"])
def test_cpu_fallback_follows_the_reference_rule_bit_for_bit(mode):
    net = _net()
    s = SIGN[mode]
    metrics = [s * v for v in METRICS]
    kb, twin = KeepBest(net, mode=mode), Twin(net, mode, s * INF)
    assert kb.value == s * INF and kb.epoch == -1 and kb.calls == 0
    taken = _run(kb, twin, net, metrics)
    assert taken == TAKEN
    assert kb.epoch == 5 and kb.calls == 7 and kb.value == s * 1.0
    _walk(net, 99)
    assert not torch.equal(net[3].weight, twin.snap["3.weight"])
    kb.restore()
    _same(net.state_dict(), twin.snap)                     # restore() gives those tensors back (buffers included)


def test_epoch_is_the_index_of_the_call_that_took():
    net = _net()
    kb = KeepBest(net)
    seen = []
    for v in METRICS:
        kb.update(v)
        seen.append(kb.epoch)
    assert seen == EPOCHS


def test_metric_forms_on_the_torch_path():
    net = _net()
    kb = KeepBest(net)
    assert int(kb.update(torch.tensor(3.0))) == 1                       # 0-d CPU tensor
    assert int(kb.update(torch.tensor([2.5], dtype=torch.float64))) == 1
    assert int(kb.update(2.5 + 1e-12)) == 1                             # compared in fp32: this IS 2.5, a tie
    assert kb.value == 2.5
    assert int(kb.update(1e39)) == 0 and int(kb.update(-1e39)) == 1 and kb.value == -INF      # (fp32 overflow -> inf)
    with pytest.raises(ValueError):
        KeepBest(net, mode="best")


def test_restore_before_any_snapshot_raises():
    net = _net()
    kb = KeepBest(net)
    with pytest.raises(_lib.MfmError, match="no snapshot"):
        kb.restore()
    kb.update(NAN)                                          # a NaN never takes: still nothing to restore
    assert kb.calls == 1 and kb.epoch == -1
    with pytest.raises(_lib.MfmError, match="no snapshot"):
        kb.restore()
    kb2 = KeepBest(net, initial=1.0)
    kb2.update(2.0)
    with pytest.raises(_lib.MfmError, match="no snapshot"):
        kb2.restore()


def test_the_references_initial_value_works():
    net = _net()
    kb, twin = KeepBest(net, initial=999999.0), Twin(net, "min", 999999.0)
    assert kb.value == 999999.0
    assert _run(kb, twin, net, [1e7, 999999.0, 3.0, 4.0]) == [0, 1, 1, 0]


def test_first_metric_inf_takes_in_mode_min():
    net = _net()
    kb = KeepBest(net)
    assert int(kb.update(INF)) == 1 and kb.epoch == 0       # inf <= inf
    kb = KeepBest(net, mode="max")
    assert int(kb.update(-INF)) == 1 and kb.epoch == 0
    kb = KeepBest(net, mode="max")
    assert int(kb.update(INF)) == 1 and int(kb.update(1e30)) == 0


@pytest.mark.parametrize("mode", ["min", "max"])
def test_state_dict_round_trips_and_the_sequence_continues(mode):
    s = SIGN[mode]
    metrics = [s * v for v in METRICS]
    net = _net()
    kb, twin = KeepBest(net, mode=mode), Twin(net, mode, s * INF)
    _run(kb, twin, net, metrics[:3])
    sd = kb.state_dict()
    assert sd["mode"] == mode and sd["value"] == s * 2.0 and sd["calls"] == 3 and sd["epoch"] == 2
    assert list(sd["snapshot"]) == list(net.state_dict())   # the model's own names
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    fresh = KeepBest(net, mode="min" if mode == "max" else "max")          # (the mode travels too)
    fresh.load_state_dict(torch.load(buf, weights_only=False))
    assert fresh.mode == mode and fresh.calls == 3 and fresh.epoch == 2 and fresh.value == s * 2.0
    _same(fresh.state_dict()["snapshot"], twin.snap)
    for k, v in enumerate(metrics[3:]):
        _walk(net, 3 + k)
        a, b, c = kb.update(v), fresh.update(v), twin.update(v)
        assert int(a) == int(b) == int(c)
        assert (fresh.value, fresh.calls, fresh.epoch) == (kb.value, kb.calls, kb.epoch) == (twin.best, twin.calls, twin.epoch)
        _same(fresh.state_dict()["snapshot"], twin.snap)
        _same(kb.state_dict()["snapshot"], twin.snap)
    assert kb.epoch == 5
    # a state without a snapshot loads too; one whose tensors are not the model's is refused
    empty = KeepBest(net).state_dict()
    assert empty["snapshot"] is None and empty["epoch"] == -1
    fresh.load_state_dict(empty)
    assert fresh.epoch == -1 and fresh.calls == 0 and fresh.value == INF
    with pytest.raises(_lib.MfmError, match="do not match"):
        KeepBest(nn.Linear(3, 2)).load_state_dict(sd)


def test_deepcopy_and_pickle_drop_the_ticket_word():
    kb = KeepBest(_net())
    kb.update(1.0)
    state = torch.zeros(_lib.MFM_KEEP_STATE_WORDS, dtype=torch.int32)
    kb._mfm_state, kb._mfm_ticket, kb._mfm_taken = state, state[4:5], state[3]      # as after a flat call
    b = copy.deepcopy(kb)
    assert b._mfm_ticket is None and b._mfm_taken is None and kb._mfm_ticket is not None
    assert b.model is not kb.model and b.value == 1.0 and b.epoch == 0
    buf = io.BytesIO()
    torch.save(kb, buf)
    buf.seek(0)
    c = torch.load(buf, weights_only=False)
    assert isinstance(c, KeepBest) and c._mfm_ticket is None and c._mfm_taken is None
    assert not any("ticket" in k for k in kb.state_dict())
    _same(c.state_dict()["snapshot"], kb.state_dict()["snapshot"])
    assert int(c.update(0.5)) == 1 and c.epoch == 1 and kb.epoch == 0              # the copy goes its own way
