"""Host-side checks of the prediction-only path: the workspace query is exact arithmetic, the new methods exist on the three
fused classes, and CPU tensors are refused (there is no CPU fallback)."""
import pytest
import torch

from factorized_amd import _lib, configs, engine
from factorized_amd import mfm_model as M
from tests import cases


def _want(T, N, h, cap):
    rows = min(N, cap) if cap > 0 else N
    return rows * T * 4 * ((h + 15) // 16 * 16) + N + 4


@pytest.mark.parametrize("name", cases.KLEF_CASES)
def test_workspace_query_is_exact_arithmetic(name):
    cs = cases.load_case(name)
    cfg = cs["cfg"]
    h = cfg["zl_size"] + cfg["za_size"] + cfg["zv_size"]
    q = _lib.lib().mfm_predict_klef_workspace_floats
    for cap in (0, 1, 4, 16, 32, 33, 64, 1024):
        assert q(cs["T"], cs["B"], h, cap) == _want(cs["T"], cs["B"], h, cap), (name, cap)


def test_workspace_query_large_split_and_bad_sizes():
    q = _lib.lib().mfm_predict_klef_workspace_floats
    assert q(50, 2048, 120, 0) == 2048 * 50 * 512 + 2048 + 4
    assert q(50, 2048, 120, 1024) == 1024 * 50 * 512 + 2048 + 4
    assert q(20, 1 << 22, 120, 0) == (1 << 22) * 20 * 512 + (1 << 22) + 4          # beyond 2^31 floats: 64-bit arithmetic
    assert q(0, 5, 120, 0) == 0 and q(5, 0, 120, 0) == 0 and q(5, 5, 0, 0) == 0 and q(5, 5, 120, -1) == 0


def test_predict_entry_validates_on_the_host():
    L = _lib.lib()
    assert L.mfm_predict_klef(0, 5, 10, 120, 32, 16, 1, 0, None, None, None, None, None, None, None, 0, None) == -1
    assert b"sizes must be positive" in L.mfm_last_error()
    assert L.mfm_predict_klef(3, 5, 10, 120, 32, 16, 1, 0, None, None, None, None, None, None, None, 0, None) == -1
    assert b"must not be null" in L.mfm_last_error()


@pytest.mark.parametrize("cls", ["MFM_KL_EF", "MFM_KL", "MFM"])
def test_methods_exist_and_cpu_tensors_are_refused(cls):
    klass = getattr(M, cls)
    assert callable(getattr(klass, "predict")) and callable(getattr(klass, "evaluate"))
    cfgs = configs.canonical_configs(dropout=False)
    model = klass(*cfgs)
    was = model.training
    x = torch.zeros(3, 2, sum(cfgs[0]["input_dims"]))
    with pytest.raises(_lib.MfmError):
        model.predict(x)
    with pytest.raises(_lib.MfmError):
        model.evaluate(x, torch.zeros(2))
    assert model.training == was


def test_engine_predict_refuses_cpu_tensors():
    assert callable(engine.MFMEngine.predict)
    e = engine.MFMEngine.__new__(engine.MFMEngine)          # (the constructor itself refuses a machine without a GPU)
    e.cfg = configs.canonical_configs(dropout=False)[0]
    e.device = torch.device("cuda")
    x = torch.zeros(3, 2, sum(e.cfg["input_dims"]))
    with pytest.raises(_lib.MfmError):
        e.predict(x)
    with pytest.raises(_lib.MfmError):
        e.predict(x, torch.zeros(2))
