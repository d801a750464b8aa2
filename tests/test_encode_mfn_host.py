"""mfm_encode_mfn without a GPU: the symbols and their prototypes, the workspace formula of include/mfm_hip.h, and the offsets
tables of engine.encode for the MFN variants."""
import ctypes as C

import pytest

from factorized_amd import _lib, configs, engine
from tests.mfn_entries import CANON_SIZES, hp as _hp, ODD_SIZES, up4 as _up4

NEW = ["mfm_encode_mfn", "mfm_encode_mfn_tile_rows", "mfm_encode_mfn_workspace_floats"]
CANON, ODD = CANON_SIZES[:17], ODD_SIZES[:17]


def _formula(T, N, sz, max_rows):
    """the workspace of mfm_encode_mfn as include/mfm_hip.h states it, term by term"""
    rows = min(N, max_rows) if max_rows > 0 else N
    zl, za, zv = sz[3:6]
    hl, ha, hv = sz[7:10]
    M, g1, g2 = sz[10], sz[14], sz[15]
    return (rows * T * 4 * (_hp(zl) + _hp(za) + _hp(zv) + _hp(hl) + _hp(ha) + _hp(hv))
            + rows * T * (_hp(hl) + _hp(ha) + _hp(hv))
            + _up4(rows * hl) + _up4(rows * ha) + _up4(rows * hv)
            + _up4(rows * T * M) + _up4(rows * T * g1) + _up4(rows * T * g2))


def _sizes(sz):
    return (C.c_int32 * 17)(*sz)


def test_symbols_and_prototypes():
    L = _lib.lib()
    for n in NEW:
        assert hasattr(L, n), n
        res, args = _lib._SIGS[n]
        assert getattr(L, n).restype == res and list(getattr(L, n).argtypes) == list(args)
    assert L.mfm_encode_mfn_workspace_floats.restype == C.c_int64
    assert list(L.mfm_encode_mfn_workspace_floats.argtypes) == [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int64]
    assert L.mfm_encode_mfn.restype == C.c_int and len(L.mfm_encode_mfn.argtypes) == 10
    assert list(L.mfm_encode_mfn.argtypes[:3]) == [C.c_int32, C.c_int64, C.POINTER(C.c_int32)]
    assert list(L.mfm_encode_mfn_tile_rows.argtypes) == [C.c_int64, C.c_int64]


@pytest.mark.parametrize("sz", [CANON, ODD])
@pytest.mark.parametrize("T,N,cap", [(20, 32, 0), (20, 1024, 1024), (7, 33, 16), (1, 1, 0), (9, 19, 4), (3, 5000, 1024)])
def test_workspace_is_the_formula_of_the_header(sz, T, N, cap):
    assert _lib.lib().mfm_encode_mfn_workspace_floats(T, N, _sizes(sz), cap) == _formula(T, N, sz, cap)


def test_workspace_is_zero_for_bad_sizes():
    L = _lib.lib()
    assert L.mfm_encode_mfn_workspace_floats(0, 5, _sizes(CANON), 0) == 0
    assert L.mfm_encode_mfn_workspace_floats(5, 0, _sizes(CANON), 0) == 0
    assert L.mfm_encode_mfn_workspace_floats(5, 5, _sizes(CANON), -1) == 0
    assert L.mfm_encode_mfn_workspace_floats(5, 5, None, 0) == 0
    for i in range(16):
        bad = list(CANON)
        bad[i] = 0
        assert L.mfm_encode_mfn_workspace_floats(5, 5, _sizes(bad), 0) == 0, i
    bad = list(CANON)
    bad[16] = 2
    assert L.mfm_encode_mfn_workspace_floats(5, 5, _sizes(bad), 0) == 0


def test_workspace_does_not_grow_with_N_beyond_the_row_cap():
    L = _lib.lib()
    at_cap = L.mfm_encode_mfn_workspace_floats(20, 64, _sizes(CANON), 64)
    assert at_cap > 0
    for N in (65, 1024, 1 << 20):
        assert L.mfm_encode_mfn_workspace_floats(20, N, _sizes(CANON), 64) == at_cap
    assert L.mfm_encode_mfn_workspace_floats(20, 32, _sizes(CANON), 64) < at_cap


def test_tile_rows_query_follows_the_six_workgroups_per_cu_rule():
    L = _lib.lib()
    cus = L.mfm_device_cus()
    assert L.mfm_encode_mfn_tile_rows(cus - 1, 0) == 1 and L.mfm_encode_mfn_tile_rows(cus, 0) == 4
    assert L.mfm_encode_mfn_tile_rows(10 * cus, cus - 1) == 1
    assert L.mfm_encode_mfn_tile_rows(0, 0) == -1 and L.mfm_encode_mfn_tile_rows(5, -1) == -1


@pytest.mark.parametrize("variant,count", [("kl", 62), ("mmd", 48)])
def test_offsets_tables_name_only_tensors_of_the_layout(variant, count):
    names = engine.MFMEngine._ENCODE_MFN_TENSORS[variant]
    shapes = engine.param_shapes(configs.canonical_configs(dropout=False), variant)
    assert len(names) == count and len(set(names)) == count
    assert all(n in shapes for n in names), [n for n in names if n not in shapes]
    assert not any(n.startswith("mfn_encoder.out_fc") for n in names)          # unused by the reference's forward
