"""Host-side checks of the gradient-based interpretation (model.influence / engine.influence_factors): the float64 reference
recursion of tests/influence_ref.py equals torch.autograd.functional.jacobian of the oracle's decoder, the package's torch
fallback (float32, CPU tensors) agrees with it element by element, the two new entries are declared, bound and exported and
validate on the host, the methods exist on the three fused classes, the result fields are views of one tensor, and a CPU model
is refused."""
import ctypes as C
import os
import re

import pytest
import torch

from factorized_amd import _infer, _lib, configs, synth
from factorized_amd import mfm_model as M
from tests import cases
from tests import influence_ref as R

NEW = ("mfm_influence_factors", "mfm_influence_factors_workspace_floats")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfm_hip.h")
_SHARED = {}


def _case(name, rows):
    """a golden case's oracle, the oracle's factors of its first `rows` rows and the float64 reference, computed once"""
    if name not in _SHARED:
        cs = cases.load_case(name)
        model = M.MFM_KL_EF(*cs["cfgs"])
        w = synth.make_weights({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1234)
        m = R.oracle_model("kl_ef", cs["cfgs"], w)
        torch.set_num_threads(4)
        z = [t[:rows].contiguous() for t in R.oracle_z(m, torch.from_numpy(cs["x"]))]
        _SHARED[name] = dict(cs=cs, m=m, z=z, ref=R.oracle_influence(m, *z, cs["T"]))
    return _SHARED[name]


@pytest.mark.parametrize("name,rows", [("klef_odd_b19_t9", 4), ("klef_b5_t1", 5)])
def test_reference_recursion_equals_autograd_jacobian(name, rows):
    s = _case(name, rows)
    cs, m = s["cs"], s["m"]
    fy, fms = R.oracle_f(m, *s["z"])
    assert s["ref"].shape == (2, 3, cs["T"], rows)
    for i, (dn, fm) in enumerate(zip(R.DECODERS, fms)):
        want = R.autograd_influence(getattr(m, dn), torch.cat([fy, fm], dim=1).double(), cs["T"], fy.shape[1])
        # (the reference computes f in float64 from z, this feeds the oracle's float32 f: compare on the same embedding)
        got = R.decoder_influence(getattr(m, dn), torch.cat([fy, fm], dim=1), cs["T"], fy.shape[1]).numpy()
        err = R.pointwise_err(got, want)
        print("influence_ref_vs_autograd %s %s %.3e" % (name, dn, err))
        assert err <= 1e-8, (dn, err)
        assert R.pointwise_err(s["ref"][:, i], want) <= 1e-4      # (float32 against float64 f)


@pytest.mark.parametrize("name,rows", [("klef_odd_b19_t9", 4), ("klef_b5_t1", 5)])
def test_torch_fallback_on_cpu_tensors_agrees_pointwise(name, rows):
    s = _case(name, rows)
    cs, m = s["cs"], s["m"]
    fy, fms = R.oracle_f(m, *s["z"])
    decs = [(d.lstm.weight_ih.detach(), d.lstm.weight_hh.detach(), d.lstm.bias_ih.detach(), d.lstm.bias_hh.detach(), d.fc1.weight.detach())
            for d in (getattr(m, dn) for dn in R.DECODERS)]
    with torch.no_grad():
        got = _infer.influence_factors_torch(decs, fy, fms, cs["T"])
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, cs["T"], rows)
    err = R.pointwise_err(got.numpy(), s["ref"])
    print("influence_fallback_cpu %s %.3e" % (name, err))
    assert err <= 1e-4, err


def test_new_entries_are_declared_bound_and_exported():
    text = open(HEADER).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.exported_names()
        assert getattr(raw, name) is not None
        assert getattr(_lib.lib(), name).argtypes is not None
    assert _lib.lib().mfm_abi_version() == 5


def _up(v):
    return (v + 15) // 16 * 16


def test_workspace_query_is_the_documented_arithmetic_and_entry_validates():
    L = _lib.lib()
    for over in ({}, cases.ODD):
        c = configs.canonical_configs(dropout=False, **over)[0]
        sizes = (C.c_int32 * 12)(c["zl_size"], c["za_size"], c["zv_size"], c["zy_size"], c["fl_size"], c["fa_size"], c["fv_size"],
                                 c["fy_size"], *c["input_dims"], c["output_dim"])
        want = 0
        for fm, d in zip((c["fl_size"], c["fa_size"], c["fv_size"]), c["input_dims"]):
            hp = _up(c["fy_size"] + fm)
            want += 8 * hp * hp + 4 * hp + _up(d) * hp
        for T, N, cap in ((7, 33, 0), (20, 1 << 22, 0), (1, 5, 4)):
            assert L.mfm_influence_factors_workspace_floats(T, N, sizes, cap) == want
        for bad in ((0, 5, 0), (5, 0, 0), (5, 5, -1)):
            assert L.mfm_influence_factors_workspace_floats(bad[0], bad[1], sizes, bad[2]) == 0
        assert L.mfm_influence_factors_workspace_floats(5, 5, None, 0) == 0
        assert L.mfm_influence_factors(0, 5, sizes, None, None, None, None, None, 0, None) == -1
        assert b"must not be null" in L.mfm_last_error()
    assert L.mfm_influence_factors(3, 5, None, None, None, None, None, None, 0, None) == -1
    assert b"must not be null" in L.mfm_last_error()


def test_influence_fields_are_views_of_one_tensor():
    from factorized_amd import engine
    assert engine.Influence is _infer.Influence and engine.Influence._fields == ("fy", "fm")
    c = configs.canonical_configs(dropout=False)[0]
    model = M.MFM_KL_EF(*configs.canonical_configs(dropout=False))
    z =[torch.randn(2, c[k], generator=torch.Generator().manual_seed(3)) for k in ("zl_size", "za_size", "zv_size", "zy_size")]
    out = model._influence_torch(*z, 2)                      # (the plain-torch path takes tensors of any device)
    assert isinstance(out, engine.Influence)
    assert tuple(out.fy.shape) == tuple(out.fm.shape) == (3, 2, 2)
    base = out.fy._base if out.fy._base is not None else out.fy
    assert out.fm._base is base and tuple(base.shape) == (2, 3, 2, 2)
    assert out.fy.data_ptr() == base.data_ptr() and out.fm.data_ptr() == base.data_ptr() + 4 * 3 * 2 * 2


@pytest.mark.parametrize("cls", ["MFM_KL_EF", "MFM_KL", "MFM"])
def test_methods_exist_and_a_cpu_model_is_refused(cls):
    klass = getattr(M, cls)
    assert callable(getattr(klass, "influence")) and callable(getattr(klass, "influence_factors"))
    from factorized_amd import engine
    assert callable(engine.MFMEngine.influence_factors) and callable(engine.MFMEngine.influence_factors_workspace_floats)
    assert _infer._ENTRIES["influence"] == ("_influence_bufs", "_influence_refused", "mfm_influence_factors")
    cfgs = configs.canonical_configs(dropout=False)
    c = cfgs[0]
    model = klass(*cfgs)
    was = model.training
    with pytest.raises(_lib.MfmError):
        model.influence(torch.zeros(3, 2, sum(c["input_dims"])))
    with pytest.raises(_lib.MfmError):
        model.influence_factors(torch.zeros(2, c["zl_size"]), torch.zeros(2, c["za_size"]), torch.zeros(2, c["zv_size"]),
                                torch.zeros(2, c["zy_size"]), 3)
    assert model.training == was


def test_mfn_has_neither():
    assert not hasattr(M.MFN, "influence") and not hasattr(M.MFN, "influence_factors")
