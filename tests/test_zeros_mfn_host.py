"""mfm_predict_zeros_mfn without a GPU: the symbols and their prototypes, the workspace formula of include/mfm_hip.h term by term,
the argument checks that run before anything touches a device, the offsets tables of engine.predict_zeros for the MFN variants,
and the fixtures against the CPU oracle."""
import ctypes as C
import os

import numpy as np
import pytest

from factorized_amd import _lib, configs, engine, synth
from tests import cases, zeros_ref
from tests.mfn_entries import CANON_SIZES as CANON, hp as _hp, odd_cfgs, ODD_SIZES as ODD, up4 as _up4

NEW = ["mfm_predict_zeros_mfn", "mfm_predict_zeros_mfn_tile_rows", "mfm_predict_zeros_mfn_workspace_floats"]


def _formula(T, N, sz, max_rows):
    """the workspace of mfm_predict_zeros_mfn as include/mfm_hip.h states it, term by term"""
    rows = min(N, max_rows) if max_rows > 0 else N
    d = sz[0:3]
    zl, za, zv = sz[3:6]
    zy = sz[6]
    hl, ha, hv = sz[7:10]
    M, g1, g2 = sz[10], sz[14], sz[15]
    fl, fa, fv, fy = sz[17:21]
    hsum = _hp(hl) + _hp(ha) + _hp(hv)
    return (max(rows * T * 4 * hsum, rows * T * (_hp(fy + fl) + _hp(fy + fa) + _hp(fy + fv)))
            + rows * T * hsum
            + _up4(rows * hl) + _up4(rows * ha) + _up4(rows * hv)
            + _up4(3 * rows * T * M) + _up4(3 * rows * T * g1) + _up4(3 * rows * T * g2)
            + T * 4 * (hsum + _hp(zl) + _hp(za) + _hp(zv))
            + T * hsum + _up4(hl) + _up4(ha) + _up4(hv)
            + _up4(rows * zl) + _up4(rows * za) + _up4(rows * zv)
            + _up4(3 * rows * zy)
            + _up4(sum(-(-T * rows // 64) * -(-dm // 64) for dm in d))
            + 12)


def _sizes(sz):
    return (C.c_int32 * 23)(*sz)


def test_symbols_and_prototypes():
    L = _lib.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in _lib.exported_names(), n
        res, args = _lib._SIGS[n]
        assert getattr(L, n).restype == res and list(getattr(L, n).argtypes) == list(args)
    assert L.mfm_predict_zeros_mfn_workspace_floats.restype == C.c_int64
    assert list(L.mfm_predict_zeros_mfn_workspace_floats.argtypes) == [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int64]
    assert list(L.mfm_predict_zeros_mfn_tile_rows.argtypes) == [C.c_int64, C.c_int64]
    # the arguments of mfm_predict_zeros_klef
    assert L.mfm_predict_zeros_mfn.restype == C.c_int
    assert list(L.mfm_predict_zeros_mfn.argtypes) == list(L.mfm_predict_zeros_klef.argtypes) and len(L.mfm_predict_zeros_mfn.argtypes) == 13


@pytest.mark.parametrize("sz", [CANON, ODD])
@pytest.mark.parametrize("T,N,cap", [(20, 32, 0), (20, 1024, 1024), (7, 33, 16), (1, 1, 0), (9, 19, 4), (3, 5000, 1024)])
def test_workspace_is_the_formula_of_the_header(sz, T, N, cap):
    assert _lib.lib().mfm_predict_zeros_mfn_workspace_floats(T, N, _sizes(sz), cap) == _formula(T, N, sz, cap)


def test_workspace_is_zero_for_bad_sizes():
    L = _lib.lib()
    f = L.mfm_predict_zeros_mfn_workspace_floats
    assert f(5, 5, _sizes(CANON), 0) > 0
    assert f(0, 5, _sizes(CANON), 0) == 0
    assert f(5, 0, _sizes(CANON), 0) == 0
    assert f(5, 5, _sizes(CANON), -1) == 0
    assert f(5, 5, None, 0) == 0
    for i in list(range(16)) + list(range(17, 22)):
        bad = list(CANON)
        bad[i] = 0
        assert f(5, 5, _sizes(bad), 0) == 0, i
    for i in (16, 22):              # heads and the loss kind: 0 or 1
        bad = list(CANON)
        bad[i] = 2
        assert f(5, 5, _sizes(bad), 0) == 0, i


def test_workspace_does_not_grow_with_N_beyond_the_row_cap():
    f = _lib.lib().mfm_predict_zeros_mfn_workspace_floats
    at_cap = f(20, 64, _sizes(CANON), 64)
    assert at_cap > 0
    for N in (65, 1024, 1 << 20):
        assert f(20, N, _sizes(CANON), 64) == at_cap
    assert f(20, 32, _sizes(CANON), 64) < at_cap


def test_tile_rows_query_follows_the_six_workgroups_per_cu_rule():
    """three recurrences per row: four-row tiles from 2 * CUs rows per chunk"""
    L = _lib.lib()
    cus = L.mfm_device_cus()
    assert L.mfm_predict_zeros_mfn_tile_rows(2 * cus - 1, 0) == 1 and L.mfm_predict_zeros_mfn_tile_rows(2 * cus, 0) == 4
    assert L.mfm_predict_zeros_mfn_tile_rows(10 * cus, 2 * cus - 1) == 1
    assert L.mfm_predict_zeros_mfn_tile_rows(0, 0) == -1 and L.mfm_predict_zeros_mfn_tile_rows(5, -1) == -1


def test_entry_validates_on_the_host():
    """T < 1, N < 1, a bad size, a null pointer and a negative row cap: -1 and a message, before any pointer is followed or any GPU
    call is made (the device pointers here are made-up addresses)."""
    L = _lib.lib()
    offs = (C.c_int64 * 100)(*[64 * i for i in range(100)])
    fake = [C.c_void_p(0x1000 * (i + 1)) for i in range(7)]       # params, x, y, workspace, y_hat, gen, disc

    def call(T=7, N=33, sizes=_sizes(CANON), params=fake[0], offsets=offs, x=fake[1], y=fake[2], ws=fake[3], y_hat=fake[4], gen=fake[5],
             disc=fake[6], max_rows=0):
        return L.mfm_predict_zeros_mfn(T, N, sizes, params, offsets, x, y, ws, y_hat, gen, disc, max_rows, None)

    zero_size = list(CANON)
    zero_size[18] = 0
    for kw, text in ((dict(T=0), b"T 0"), (dict(N=0), b"N 0"), (dict(sizes=None), b"sizes must be positive"),
                     (dict(sizes=_sizes(zero_size)), b"sizes must be positive"), (dict(params=None), b"must not be null"),
                     (dict(offsets=None), b"must not be null"), (dict(x=None), b"must not be null"), (dict(ws=None), b"must not be null"),
                     (dict(y_hat=None), b"must not be null"), (dict(gen=None), b"must not be null"),
                     (dict(disc=None), b"come together"), (dict(y=None), b"come together"), (dict(max_rows=-1), b"row cap -1")):
        assert call(**kw) == -1, kw
        msg = L.mfm_last_error()
        assert b"predict zeros mfn" in msg and text in msg, (kw, msg)


@pytest.mark.parametrize("variant,count", [("kl", 100), ("mmd", 86)])
def test_offsets_tables_name_only_tensors_of_the_layout(variant, count):
    names = engine.MFMEngine._ENCODE_MFN_TENSORS[variant] + engine.MFMEngine._DECODE_TENSORS
    shapes = engine.param_shapes(configs.canonical_configs(dropout=False), variant)
    assert len(names) == count and len(set(names)) == count
    assert all(n in shapes for n in names), [n for n in names if n not in shapes]


def test_entries_table_keeps_a_cache_of_its_own():
    from factorized_amd import _infer
    assert _infer._ENTRIES["zeros_mfn"] == ("_zeros_mfn_bufs", "_zeros_mfn_refused", "mfm_predict_zeros_mfn")
    assert _infer._ENTRIES["zeros"] == ("_zeros_bufs", "_zeros_refused", "mfm_predict_zeros_klef")


@pytest.mark.parametrize("variant", ["kl", "mmd"])
def test_oracle_on_zeroed_inputs_reproduces_the_fixture(variant):
    """pins the fixtures (the reference's own run, tests/golden/make_golden_zeros_mfn.py) and the oracle to each other"""
    cfgs = odd_cfgs()
    cfg = cfgs[0]
    gold = np.load(os.path.join(cases.GOLDEN, "%s_zeros_b19_t9.npz" % variant))
    B, T = [int(v) for v in gold["meta"]]
    assert (B, T) == (19, 9)
    xn, yn = synth.make_batch(cfg["input_dims"], B, T, seed=7, output_dim=cfg["output_dim"])
    from oracle import mfm_oracle as O
    w = synth.make_weights(O.state_shapes(O.build(variant, cfgs)), seed=1234)
    ref = zeros_ref.oracle_zeros(variant, cfgs, w, xn, yn)
    assert ref["y_hat"].shape == gold["y_hat"].shape == (3, B, cfg["output_dim"])
    assert cases.rel_err(ref["y_hat"], gold["y_hat"]) <= 1e-6
    for k in ("gen", "disc"):
        for c in range(3):
            assert abs(ref[k][c] - gold[k][c]) <= 1e-6 * abs(gold[k][c]), (k, c, ref[k][c], gold[k][c])
