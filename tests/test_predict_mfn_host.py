"""mfm_predict_mfn without a GPU: the symbols and their prototypes, the workspace formula of include/mfm_hip.h term by term, the
argument checks that run before anything touches a device, the offsets table of engine.predict(label_only=True), and the
refusal of CPU tensors."""
import ctypes as C

import pytest
import torch

from factorized_amd import _lib, configs, engine
from factorized_amd import mfm_model as M
from tests.mfn_entries import CANON_SIZES as CANON, hp as _hp, ODD_SIZES as ODD, up4 as _up4

NEW = ["mfm_predict_mfn", "mfm_predict_mfn_tile_rows", "mfm_predict_mfn_workspace_floats"]


def _formula(T, N, sz, max_rows):
    """the workspace of mfm_predict_mfn as include/mfm_hip.h states it, term by term"""
    rows = min(N, max_rows) if max_rows > 0 else N
    hl, ha, hv = sz[7:10]
    M_, g1, g2 = sz[10], sz[14], sz[15]
    hsum = _hp(hl) + _hp(ha) + _hp(hv)
    return (rows * T * 4 * hsum
            + rows * T * hsum
            + _up4(rows * hl) + _up4(rows * ha) + _up4(rows * hv)
            + _up4(rows * T * M_) + _up4(rows * T * g1) + _up4(rows * T * g2)
            + _up4(rows)
            + 4)


def _sizes(sz):
    return (C.c_int32 * 23)(*sz)


def test_symbols_and_prototypes():
    L = _lib.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in _lib.exported_names(), n
        res, args = _lib._SIGS[n]
        assert getattr(L, n).restype == res and list(getattr(L, n).argtypes) == list(args)
    assert L.mfm_predict_mfn_workspace_floats.restype == C.c_int64
    assert list(L.mfm_predict_mfn_workspace_floats.argtypes) == [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int64]
    assert list(L.mfm_predict_mfn_tile_rows.argtypes) == [C.c_int64, C.c_int64]
    assert L.mfm_predict_mfn.restype == C.c_int and len(L.mfm_predict_mfn.argtypes) == 12


def test_the_header_declares_the_three_entries():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "mfm_hip.h")) as f:
        text = f.read()
    for n in NEW:
        assert " %s(" % n in text, n


@pytest.mark.parametrize("sz", [CANON, ODD])
@pytest.mark.parametrize("T,N,cap", [(20, 32, 0), (20, 1024, 1024), (7, 33, 16), (1, 1, 0), (9, 19, 4), (3, 5000, 1024)])
def test_workspace_is_the_formula_of_the_header(sz, T, N, cap):
    assert _lib.lib().mfm_predict_mfn_workspace_floats(T, N, _sizes(sz), cap) == _formula(T, N, sz, cap)


def test_workspace_is_zero_for_bad_sizes():
    f = _lib.lib().mfm_predict_mfn_workspace_floats
    assert f(5, 5, _sizes(CANON), 0) > 0
    assert f(0, 5, _sizes(CANON), 0) == 0
    assert f(5, 0, _sizes(CANON), 0) == 0
    assert f(5, 5, _sizes(CANON), -1) == 0
    assert f(5, 5, None, 0) == 0
    for i in list(range(16)) + list(range(17, 22)):      # the encoders' z sizes and fl / fa / fv too: positive, otherwise unused
        bad = list(CANON)
        bad[i] = 0
        assert f(5, 5, _sizes(bad), 0) == 0, i
        bad[i] = -3
        assert f(5, 5, _sizes(bad), 0) == 0, i
    for i in (16, 22):              # heads and the loss kind: 0 or 1
        for v in (2, -1):
            bad = list(CANON)
            bad[i] = v
            assert f(5, 5, _sizes(bad), 0) == 0, (i, v)


def test_heads_word_does_not_change_the_workspace():
    f = _lib.lib().mfm_predict_mfn_workspace_floats
    other = list(CANON)
    other[16] = 0
    assert f(20, 229, _sizes(CANON), 64) == f(20, 229, _sizes(other), 64)


@pytest.mark.parametrize("T,N,cap", [(20, 32, 0), (20, 229, 0), (20, 1024, 1024), (7, 33, 16)])
def test_workspace_is_smaller_than_that_of_encode(T, N, cap):
    """encode of these classes carries three more projections (the encoders')"""
    L = _lib.lib()
    mine = L.mfm_predict_mfn_workspace_floats(T, N, _sizes(CANON), cap)
    enc = L.mfm_encode_mfn_workspace_floats(T, N, (C.c_int32 * 17)(*CANON[:17]), cap)
    assert 0 < mine < enc


def test_workspace_does_not_grow_with_N_beyond_the_row_cap():
    f = _lib.lib().mfm_predict_mfn_workspace_floats
    at_cap = f(20, 64, _sizes(CANON), 64)
    assert at_cap > 0
    for N in (65, 1024, 1 << 20):
        assert f(20, N, _sizes(CANON), 64) == at_cap
    assert f(20, 32, _sizes(CANON), 64) < at_cap


def test_tile_rows_query_follows_the_six_workgroups_per_cu_rule():
    """three recurrences per row: four-row tiles from 2 * CUs rows per chunk"""
    L = _lib.lib()
    cus = L.mfm_device_cus()
    assert L.mfm_predict_mfn_tile_rows(2 * cus - 1, 0) == 1 and L.mfm_predict_mfn_tile_rows(2 * cus, 0) == 4
    assert L.mfm_predict_mfn_tile_rows(10 * cus, 2 * cus - 1) == 1
    assert L.mfm_predict_mfn_tile_rows(0, 0) == -1 and L.mfm_predict_mfn_tile_rows(5, -1) == -1


def test_entry_validates_on_the_host():
    """T < 1, N < 1, a bad size, a null pointer, labels without loss or loss without labels and a negative row cap: -1 and a
    message, before any pointer is followed or any GPU call is made (the device pointers here are made-up addresses)."""
    L = _lib.lib()
    offs = (C.c_int64 * 38)(*[64 * i for i in range(38)])
    fake = [C.c_void_p(0x1000 * (i + 1)) for i in range(6)]       # params, x, y, workspace, y_hat, loss

    def call(T=7, N=33, sizes=_sizes(CANON), params=fake[0], offsets=offs, x=fake[1], y=fake[2], ws=fake[3], y_hat=fake[4],
             loss=fake[5], max_rows=0):
        return L.mfm_predict_mfn(T, N, sizes, params, offsets, x, y, ws, y_hat, loss, max_rows, None)

    zero_size = list(CANON)
    zero_size[18] = 0
    for kw, text in ((dict(T=0), b"T 0"), (dict(N=0), b"N 0"), (dict(sizes=None), b"sizes must be positive"),
                     (dict(sizes=_sizes(zero_size)), b"sizes must be positive"), (dict(params=None), b"must not be null"),
                     (dict(offsets=None), b"must not be null"), (dict(x=None), b"must not be null"), (dict(ws=None), b"must not be null"),
                     (dict(y_hat=None), b"must not be null"), (dict(loss=None), b"come together"), (dict(y=None), b"come together"),
                     (dict(max_rows=-1), b"row cap -1")):
        assert call(**kw) == -1, kw
        msg = L.mfm_last_error()
        assert b"predict mfn" in msg and text in msg, (kw, msg)


@pytest.mark.parametrize("variant", ["kl", "mmd"])
def test_offsets_table_names_only_tensors_of_the_layout(variant):
    names = engine.MFMEngine._PREDICT_MFN_TENSORS
    shapes = engine.param_shapes(configs.canonical_configs(dropout=False), variant)
    assert len(names) == 38 and len(set(names)) == 38
    assert all(n in shapes for n in names), [n for n in names if n not in shapes]
    assert names[:28] == engine.MFMEngine._MFN_TENSORS and names[28] == "last_to_zy_fc1.weight"
    assert names[30:] == ("zy_to_fy_fc1.weight", "zy_to_fy_fc1.bias", "zy_to_fy_fc2.weight", "zy_to_fy_fc2.bias",
                          "fy_to_y_fc1.weight", "fy_to_y_fc1.bias", "fy_to_y_fc2.weight", "fy_to_y_fc2.bias")
    dead = [n for n in shapes if n not in names]
    assert any(n.startswith("encoder_l.") for n in dead) and any(n.startswith("decoder_v.") for n in dead)


def test_entries_table_keeps_a_cache_of_its_own():
    from factorized_amd import _infer
    assert _infer._ENTRIES["predict_mfn"] == ("_predict_mfn_bufs", "_predict_mfn_refused", "mfm_predict_mfn")
    assert _infer._ENTRIES["predict"] == ("_predict_bufs", "_predict_refused", "mfm_predict_klef")


@pytest.mark.parametrize("cls", ["MFM_KL_EF", "MFM_KL", "MFM"])
def test_label_only_refuses_cpu_tensors(cls):
    klass = getattr(M, cls)
    cfgs = configs.canonical_configs(dropout=False)
    model = klass(*cfgs)
    was = model.training
    x = torch.zeros(3, 2, sum(cfgs[0]["input_dims"]))
    with pytest.raises(_lib.MfmError):
        model.predict(x, label_only=True)
    with pytest.raises(_lib.MfmError):
        model.evaluate(x, torch.zeros(2), label_only=True)
    with pytest.raises(_lib.MfmError):
        model.evaluate(x, torch.zeros(2), torch.nn.MSELoss(), label_only=True)
    assert model.training == was


@pytest.mark.parametrize("variant", ["kl", "mmd", "kl_ef"])
def test_engine_label_only_refuses_cpu_tensors(variant):
    e = engine.MFMEngine.__new__(engine.MFMEngine)          # (the constructor itself refuses a machine without a GPU)
    e.cfg = configs.canonical_configs(dropout=False)[0]
    e.device = torch.device("cuda")
    e.variant = variant
    x = torch.zeros(3, 2, sum(e.cfg["input_dims"]))
    with pytest.raises(_lib.MfmError):
        e.predict(x, label_only=True)
    with pytest.raises(_lib.MfmError):
        e.predict(x, torch.zeros(2), label_only=True)
    assert not e.__dict__.get("_predict_mfn_bufs")
