"""Host-side checks of surrogate inference (MFM_missing.impute, mfm_impute_missing): the new symbols in the header, the library
and the binding; the entry's argument checks, which answer before anything touches a device; the module's refusals on the CPU
and its unchanged state_dict surface.  No GPU compute here."""
import ctypes as C
import os
import re

import pytest
import torch

from factorized_amd import _lib, configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mfm_impute_missing", "mfm_impute_missing_tile_rows", "mfm_impute_missing_workspace_floats"]
SIZES = [32, 8, 80, 32, 88, 8, 8, 16, 300, 5, 20, 1]          # zl za zv zy fl fa fv fy d_l d_a d_v output_dim


def _declared():
    src = open(os.path.join(ROOT, "include", "mfm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))


def test_new_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    declared, bound = _declared(), set(_lib.exported_names())
    for n in NEW:
        assert n in declared, "include/mfm_hip.h does not declare %s" % n
        assert hasattr(L, n), "libmfm_hip.so does not export %s" % n
        assert n in bound, "_lib.py does not bind %s" % n
    assert declared == bound


def test_abi_version_is_still_5():
    assert _lib.lib().mfm_abi_version() == 5 == _lib.ABI_VERSION


def test_workspace_query():
    L = _lib.lib()
    sz = (C.c_int32 * 12)(*SIZES)
    T, N = 20, 33
    hp = lambda h: (h + 15) // 16 * 16
    up4 = lambda v: (v + 3) // 4 * 4

    def case(m, rows):
        z, f = SIZES[m], SIZES[4 + m]
        pair = sum(SIZES[8:11]) - SIZES[8 + m]
        return (rows * T * 4 * (hp(z) + hp(32)) + up4(rows * z) + up4(rows * 32) + rows * T * hp(16 + f)
                + rows * T * (up4(pair) + 4))
    for m in range(3):
        assert L.mfm_impute_missing_workspace_floats(T, N, sz, 1 << m, 0) == case(m, N)
        assert L.mfm_impute_missing_workspace_floats(T, N, sz, 1 << m, 5) == case(m, 5)
    assert L.mfm_impute_missing_workspace_floats(T, N, sz, 7, 0) == sum(case(m, N) for m in range(3))
    assert L.mfm_impute_missing_workspace_floats(T, N, sz, 7, 1000) == sum(case(m, N) for m in range(3))
    for bad in ((0, N, 7, 0), (T, 0, 7, 0), (T, N, 0, 0), (T, N, 3, 0), (T, N, 8, 0), (T, N, 7, -1)):
        assert L.mfm_impute_missing_workspace_floats(bad[0], bad[1], sz, bad[2], bad[3]) == 0
    assert L.mfm_impute_missing_workspace_floats(T, N, None, 7, 0) == 0
    zero = (C.c_int32 * 12)(*[0 if i == 5 else v for i, v in enumerate(SIZES)])
    assert L.mfm_impute_missing_workspace_floats(T, N, zero, 7, 0) == 0


def _call(T=4, N=6, sizes=SIZES, cases=7, params=None, x=0x1000, ws=0x2000, out=None, cap=0, null=()):
    """mfm_impute_missing on made-up (aligned, never dereferenced) addresses: every call here must be refused by the argument
    checks, which come before any launch"""
    L = _lib.lib()
    sz = None if "sizes" in null else (C.c_int32 * 12)(*sizes)
    prm = None if "params" in null else (C.c_void_p * 74)(*(params or [0x10000 + 64 * i for i in range(74)]))
    o = None if "out" in null else (C.c_void_p * 6)(*(out or [0x90000 + 64 * i for i in range(6)]))
    rc = L.mfm_impute_missing(T, N, sz, cases, prm, C.c_void_p(x), C.c_void_p(ws), o, cap, None)
    return rc, L.mfm_last_error().decode()


def test_argument_checks_answer_without_a_device():
    ptrs = [0x10000 + 64 * i for i in range(74)]
    for null in ("sizes", "params", "out"):
        rc, msg = _call(null=(null,))
        assert rc == -1 and "must not be null" in msg, (null, msg)
    rc, msg = _call(x=0)
    assert rc == -1 and "must not be null" in msg
    rc, msg = _call(ws=0)
    assert rc == -1 and "must not be null" in msg
    rc, msg = _call(params=[0 if i == 30 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 8 of case 1 is null" in msg, msg
    rc, msg = _call(params=[0 if i == 70 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "shared parameter 4" in msg, msg
    rc, msg = _call(out=[0 if i == 3 else 0x90000 + 64 * i for i in range(6)])
    assert rc == -1 and "output of case 1 is null" in msg, msg
    # ... but what a case that was not asked for would use is not looked at
    rc, msg = _call(cases=1, N=1 << 24, params=[0 if 22 <= i < 66 else p for i, p in enumerate(ptrs)],
                    out=[0x90000, 0x90040, 0, 0, 0, 0])
    assert rc == -1 and "2^24" in msg, msg
    for kw, word in ((dict(T=0), "T 0"), (dict(N=0), "N 0"), (dict(sizes=[0 if i == 2 else v for i, v in enumerate(SIZES)]), "size 2 is 0"),
                     (dict(sizes=[-3 if i == 11 else v for i, v in enumerate(SIZES)]), "size 11 is -3"), (dict(cap=-1), "row cap -1"),
                     (dict(cases=0), "cases = 0"), (dict(cases=5), "cases = 5")):
        rc, msg = _call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    # a misaligned LSTM weight (16 bytes), a misaligned bias (4 bytes), a misaligned x
    rc, msg = _call(params=[p + 4 if i == 17 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 17 of case 0 is misaligned" in msg, msg
    rc, msg = _call(params=[p + 2 if i == 2 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 2 of case 0 is misaligned" in msg, msg
    rc, msg = _call(params=[p + 4 if i == 2 else p for i, p in enumerate(ptrs)], N=1 << 24)       # (a bias on 4 bytes is fine)
    assert rc == -1 and "2^24" in msg, msg
    rc, msg = _call(x=0x1002)
    assert rc == -1 and "x must be 4-byte aligned" in msg, msg
    rc, msg = _call(ws=0x2004)
    assert rc == -1 and "workspace 16-byte aligned" in msg, msg
    rc, msg = _call(x=0x1004, N=1 << 24)                       # (x on 4 bytes is fine: any contiguous view of a float tensor)
    assert rc == -1 and "2^24" in msg, msg
    rc, msg = _call(N=1 << 24)
    assert rc == -1 and "2^24" in msg and str(1 << 24) in msg, msg
    # a chunk whose products would pass 2^31 elements asks for a row cap
    rc, msg = _call(T=4000, N=(1 << 24) - 1)
    assert rc == -1 and "pass a row cap" in msg, msg


def test_tile_rows_query_follows_the_six_workgroups_per_cu_rule():
    L = _lib.lib()
    cus = L.mfm_device_cus()
    r = (C.c_int32 * 2)()
    n = 3 * cus                                   # two LSTMs: exactly six workgroups per CU
    assert L.mfm_impute_missing_tile_rows(n - 1, 1, 0, r) == 0 and list(r) == [1, 1]
    assert L.mfm_impute_missing_tile_rows(n, 2, 0, r) == 0 and list(r) == [4, 1]
    assert L.mfm_impute_missing_tile_rows(6 * cus, 4, 0, r) == 0 and list(r) == [4, 4]
    assert L.mfm_impute_missing_tile_rows(cus, 7, 0, r) == 0 and list(r) == [4, 1]
    assert L.mfm_impute_missing_tile_rows(6 * cus, 7, cus - 1, r) == 0 and list(r) == [1, 1]
    assert L.mfm_impute_missing_tile_rows(0, 7, 0, r) == -1
    assert L.mfm_impute_missing_tile_rows(5, 6, 0, r) == -1
    assert L.mfm_impute_missing_tile_rows(5, 7, 0, None) == -1


def test_impute_on_a_cpu_model_raises():
    from factorized_amd import mfm_model as M
    cfgs = configs.canonical_configs(dropout=False)
    model = M.MFM_missing(*cfgs)
    x = torch.zeros(3, 2, sum(cfgs[0]["input_dims"]))
    with pytest.raises(_lib.MfmError, match="move the model to the GPU"):
        model.impute(x, "l")
    with pytest.raises(_lib.MfmError, match="move the model to the GPU"):
        model.impute(x, "each")
    with pytest.raises(ValueError, match="'l', 'a', 'v' or 'each'"):
        model.impute(x, "x")


def test_state_dict_keys_are_unchanged_by_the_feature():
    from factorized_amd import mfm_model as M
    from oracle import mfm_oracle_extra as X
    cfgs = configs.canonical_configs(dropout=False)
    model = M.MFM_missing(*cfgs)
    keys = list(model.state_dict().keys())
    assert keys == list(X.CLASSES["MFM_missing"](*cfgs).state_dict().keys())
    assert model._impute_sizes() == tuple(SIZES)
    assert len(model._impute_params(("l", "a", "v"))) == 74
    single = model._impute_params(("a",))
    assert [p is None for p in single] == [not (22 <= i < 44 or i >= 66) for i in range(74)]
    with pytest.raises(_lib.MfmError):
        model.impute(torch.zeros(3, 2, 325), "v")
    assert list(model.state_dict().keys()) == keys
    assert not [k for k in model.__dict__ if k.startswith("_impute")]          # (nothing was cached on the way to the refusal)
