"""Host-side checks of encode / decode: the four new entries are declared, bound and exported, the workspace queries are the
arithmetic the header documents, the methods exist on the three fused classes (and not on MFN), and a CPU model is refused."""
import ctypes as C
import os
import re

import pytest
import torch

from factorized_amd import _lib, configs
from factorized_amd import mfm_model as M
from tests import cases

NEW = ("mfm_encode_klef", "mfm_encode_klef_workspace_floats", "mfm_decode_factors", "mfm_decode_factors_workspace_floats")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfm_hip.h")


def _up(v):
    return (v + 15) // 16 * 16


def _want_enc(T, N, zl, za, zv, cap):
    rows = min(N, cap) if cap > 0 else N
    return rows * T * 4 * (_up(zl) + _up(za) + _up(zv) + _up(zl + za + zv))


def _want_dec(T, N, fy, fl, fa, fv, cap):
    rows = min(N, cap) if cap > 0 else N
    return rows * T * (_up(fy + fl) + _up(fy + fa) + _up(fy + fv))


def test_new_entries_are_declared_bound_and_exported():
    text = open(HEADER).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.exported_names()
        assert getattr(raw, name) is not None
        assert getattr(_lib.lib(), name).argtypes is not None
    assert _lib.lib().mfm_abi_version() == 5


@pytest.mark.parametrize("name", cases.KLEF_CASES)
def test_workspace_queries_are_the_documented_arithmetic(name):
    cs = cases.load_case(name)
    c, T, N = cs["cfg"], cs["T"], cs["B"]
    qe, qd = _lib.lib().mfm_encode_klef_workspace_floats, _lib.lib().mfm_decode_factors_workspace_floats
    for cap in (0, 1, 4, 32, 33, 1000):
        assert qe(T, N, c["zl_size"], c["za_size"], c["zv_size"], cap) == _want_enc(T, N, c["zl_size"], c["za_size"], c["zv_size"], cap)
        assert qd(T, N, c["fy_size"], c["fl_size"], c["fa_size"], c["fv_size"], cap) == \
            _want_dec(T, N, c["fy_size"], c["fl_size"], c["fa_size"], c["fv_size"], cap)


def test_workspace_queries_large_split_and_bad_sizes():
    qe, qd = _lib.lib().mfm_encode_klef_workspace_floats, _lib.lib().mfm_decode_factors_workspace_floats
    assert qe(20, 1 << 22, 32, 8, 80, 0) == (1 << 22) * 20 * 4 * (32 + 16 + 80 + 128)          # beyond 2^31 floats
    assert qd(20, 1 << 22, 16, 88, 8, 8, 0) == (1 << 22) * 20 * (112 + 32 + 32)
    assert qe(20, 229, 32, 8, 80, 64) == 64 * 20 * 4 * 256
    for bad in ((0, 5, 32, 8, 80, 0), (5, 0, 32, 8, 80, 0), (5, 5, 0, 8, 80, 0), (5, 5, 32, 8, 80, -1)):
        assert qe(*bad) == 0
    for bad in ((0, 5, 16, 88, 8, 8, 0), (5, 0, 16, 88, 8, 8, 0), (5, 5, 16, 0, 8, 8, 0), (5, 5, 16, 88, 8, 8, -1)):
        assert qd(*bad) == 0


def test_entries_validate_on_the_host():
    L = _lib.lib()
    assert L.mfm_encode_klef(0, 5, 300, 5, 20, 32, 8, 80, 32, None, None, None, None, None, 0, None) == -1
    assert b"sizes must be positive" in L.mfm_last_error()
    assert L.mfm_encode_klef(3, 5, 300, 5, 20, 32, 8, 80, 32, None, None, None, None, None, 0, None) == -1
    assert b"must not be null" in L.mfm_last_error()
    assert L.mfm_decode_factors(3, 5, None, None, None, None, None, None, 0, None) == -1
    assert b"must not be null" in L.mfm_last_error()


@pytest.mark.parametrize("cls", ["MFM_KL_EF", "MFM_KL", "MFM"])
def test_methods_exist_and_a_cpu_model_is_refused(cls):
    klass = getattr(M, cls)
    assert callable(getattr(klass, "encode")) and callable(getattr(klass, "decode"))
    cfgs = configs.canonical_configs(dropout=False)
    c = cfgs[0]
    model = klass(*cfgs)
    was = model.training
    with pytest.raises(_lib.MfmError):
        model.encode(torch.zeros(3, 2, sum(c["input_dims"])))
    with pytest.raises(_lib.MfmError):
        model.decode(torch.zeros(2, c["zl_size"]), torch.zeros(2, c["za_size"]), torch.zeros(2, c["zv_size"]),
                     torch.zeros(2, c["zy_size"]), 3)
    assert model.training == was


def test_mfn_has_neither():
    assert not hasattr(M.MFN, "encode") and not hasattr(M.MFN, "decode")
