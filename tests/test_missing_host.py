"""Host-side checks of the missing-modality test protocol (predict_missing, mfm_predict_missing): the new symbols in the header,
the library and the binding; the workspace and tile-row queries; the entry's argument checks, which answer before anything
touches a device; the modules' refusals on the CPU, their pickling and their unchanged state_dict surface.  No GPU compute here."""
import ctypes as C
import os
import pickle
import re

import pytest
import torch

from factorized_amd import _lib, configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mfm_predict_missing", "mfm_predict_missing_tile_rows", "mfm_predict_missing_workspace_floats"]
SIZES = [32, 8, 80, 32, 88, 8, 8, 16, 300, 5, 20, 1]          # zl za zv zy fl fa fv fy d_l d_a d_v output_dim
CLASSES = ("MFM_missing", "seq2seq", "basic_missing")


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


def test_the_header_documents_the_parameter_table_per_family():
    src = open(os.path.join(ROOT, "include", "mfm_hip.h")).read()
    doc = src[src.index("The missing-modality test protocol"):src.index("int64_t mfm_predict_missing_workspace_floats")]
    for word in ("family 0, MFM_missing", "family 1, seq2seq", "family 2, basic_missing", "74 DEVICE pointers", "enqueue nothing",
                 "may be null"):
        assert word in doc, word


def test_workspace_query():
    L = _lib.lib()
    sz = (C.c_int32 * 12)(*SIZES)
    T, N = 20, 33
    hp = lambda h: (h + 15) // 16 * 16
    up4 = lambda v: (v + 3) // 4 * 4
    cdiv = lambda a, b: (a + b - 1) // b

    def want(family, ms, rows):
        f = 0
        for m in ms:
            z, fm, d = SIZES[m], SIZES[4 + m], SIZES[8 + m]
            f += rows * T * (up4(sum(SIZES[8:11]) - d) + 4)
            if family != 2:
                f += rows * T * 4 * hp(z) + up4(rows * z) + rows * T * hp((16 if family == 0 else 0) + fm)
            if family != 1:
                f += rows * T * 4 * hp(32)
            if family == 0:
                f += up4(rows * 32)
        if family != 2:
            f += up4(sum(cdiv(T * rows, 64) * cdiv(SIZES[8 + m], 64) for m in ms))
        return f + 12 + 4

    for family in range(3):
        for labels in (0, 1):
            for m in range(3):
                assert L.mfm_predict_missing_workspace_floats(T, N, sz, family, 1 << m, labels, 0) == want(family, [m], N)
                assert L.mfm_predict_missing_workspace_floats(T, N, sz, family, 1 << m, labels, 5) == want(family, [m], 5)
            assert L.mfm_predict_missing_workspace_floats(T, N, sz, family, 7, labels, 0) == want(family, [0, 1, 2], N)
            assert L.mfm_predict_missing_workspace_floats(T, N, sz, family, 7, labels, 1000) == want(family, [0, 1, 2], N)
    # family 0 keeps everything mfm_impute_missing does
    for cases in (1, 2, 4, 7):
        for cap in (0, 5):
            assert (L.mfm_predict_missing_workspace_floats(T, N, sz, 0, cases, 1, cap)
                    >= L.mfm_impute_missing_workspace_floats(T, N, sz, cases, cap) > 0)
    for bad in ((0, N, 0, 7, 0), (T, 0, 0, 7, 0), (T, N, 0, 0, 0), (T, N, 0, 3, 0), (T, N, 0, 8, 0), (T, N, 0, 7, -1), (T, N, 3, 7, 0),
                (T, N, 5, 7, 0), (T, N, -1, 7, 0)):
        assert L.mfm_predict_missing_workspace_floats(bad[0], bad[1], sz, bad[2], bad[3], 1, bad[4]) == 0, bad
    assert L.mfm_predict_missing_workspace_floats(T, N, None, 0, 7, 1, 0) == 0
    zero = (C.c_int32 * 12)(*[0 if i == 5 else v for i, v in enumerate(SIZES)])
    assert L.mfm_predict_missing_workspace_floats(T, N, zero, 0, 7, 1, 0) == 0


def test_tile_rows_query_follows_the_six_workgroups_per_cu_rule():
    """gen_tile_rows: one-row tiles while LSTMs x rows of a launch stay below six per CU, else four-row tiles.  The encoders'
    launch holds two LSTMs per case for family 0 and one for families 1 and 2; the decoders' one per case; family 2 has none"""
    L = _lib.lib()
    cus = L.mfm_device_cus()
    r = (C.c_int32 * 2)()

    def q(N, family, cases, cap=0):
        assert L.mfm_predict_missing_tile_rows(N, family, cases, cap, r) == 0
        return list(r)
    n = 3 * cus                                   # family 0, one case: two encoder LSTMs, exactly six workgroups per CU
    assert q(n - 1, 0, 1) == [1, 1] and q(n, 0, 2) == [4, 1] and q(6 * cus, 0, 4) == [4, 4]
    assert q(cus - 1, 0, 7) == [1, 1] and q(cus, 0, 7) == [4, 1] and q(2 * cus, 0, 7) == [4, 4]
    assert q(6 * cus - 1, 1, 1) == [1, 1] and q(6 * cus, 1, 2) == [4, 4]
    assert q(2 * cus - 1, 1, 7) == [1, 1] and q(2 * cus, 1, 7) == [4, 4]
    assert q(6 * cus - 1, 2, 4) == [1, 0] and q(6 * cus, 2, 1) == [4, 0]
    assert q(2 * cus - 1, 2, 7) == [1, 0] and q(2 * cus, 2, 7) == [4, 0]
    for family in range(3):
        assert q(6 * cus, family, 7, cus // 3 - 1)[0] == 1      # (the row cap counts, not N)
        # ... and agrees with the query of mfm_impute_missing where the launches are the same
    ri = (C.c_int32 * 2)()
    for N in (cus - 1, cus, 2 * cus, 3 * cus, 6 * cus):
        for cases in (1, 2, 4, 7):
            assert L.mfm_impute_missing_tile_rows(N, cases, 0, ri) == 0
            assert q(N, 0, cases) == list(ri)
            assert q(N, 1, cases) == [ri[1], ri[1]] and q(N, 2, cases) == [ri[1], 0]
    assert L.mfm_predict_missing_tile_rows(0, 0, 7, 0, r) == -1
    assert L.mfm_predict_missing_tile_rows(5, 0, 6, 0, r) == -1
    assert L.mfm_predict_missing_tile_rows(5, 3, 7, 0, r) == -1
    assert L.mfm_predict_missing_tile_rows(5, 0, 7, -1, r) == -1
    assert L.mfm_predict_missing_tile_rows(5, 0, 7, 0, None) == -1


def _call(T=4, N=6, sizes=SIZES, family=0, cases=7, loss=0, params=None, x=0x1000, y=0x3000, ws=0x2000, y_hat=0x90000, gen=0x91000,
          disc=0x92000, cap=0, null=()):
    """mfm_predict_missing on made-up (aligned, never dereferenced) addresses: every call here must be refused by the argument
    checks, which come before any launch"""
    L = _lib.lib()
    sz = None if "sizes" in null else (C.c_int32 * 12)(*sizes)
    prm = None if "params" in null else (C.c_void_p * 74)(*(params or [0x10000 + 64 * i for i in range(74)]))
    rc = L.mfm_predict_missing(T, N, sz, family, cases, loss, prm, C.c_void_p(x), C.c_void_p(y), C.c_void_p(ws), C.c_void_p(y_hat),
                               C.c_void_p(gen), C.c_void_p(disc), cap, None)
    return rc, L.mfm_last_error().decode()


def test_argument_checks_answer_without_a_device():
    ptrs = [0x10000 + 64 * i for i in range(74)]
    for null in ("sizes", "params"):
        rc, msg = _call(null=(null,))
        assert rc == -1 and "must not be null" in msg, (null, msg)
    for kw in (dict(x=0), dict(ws=0)):
        rc, msg = _call(**kw)
        assert rc == -1 and "must not be null" in msg, (kw, msg)
    for kw, word in ((dict(cases=3), "cases = 3"), (dict(cases=0), "cases = 0"), (dict(family=5), "family = 5"), (dict(family=-1), "family = -1"),
                     (dict(cap=-1), "row cap -1"), (dict(T=0), "T 0"), (dict(N=0), "N 0"), (dict(loss=2), "loss kind 2"),
                     (dict(sizes=[0 if i == 2 else v for i, v in enumerate(SIZES)]), "size 2 is 0"), (dict(N=1 << 24), "2^24")):
        for family in ((kw["family"],) if "family" in kw else range(3)):
            rc, msg = _call(**dict(kw, family=family))
            assert rc == -1 and word in msg, (kw, family, msg)
    # the outputs a family has must be there; labels and disc come together
    rc, msg = _call(family=0, gen=0)
    assert rc == -1 and "gen must not be null" in msg, msg
    rc, msg = _call(family=1, gen=0)
    assert rc == -1 and "gen must not be null" in msg, msg
    rc, msg = _call(family=2, y_hat=0)
    assert rc == -1 and "y_hat must not be null" in msg, msg
    for family in (0, 2):
        for kw in (dict(y=0), dict(disc=0)):
            rc, msg = _call(family=family, **kw)
            assert rc == -1 and "labels and disc come together" in msg, (family, kw, msg)
    # ... and those it does not have are not looked at (the call gets as far as the row check)
    rc, msg = _call(family=1, y=0, y_hat=0, disc=0x92000, T=4000, N=(1 << 24) - 1)
    assert rc == -1 and "pass a row cap" in msg, msg
    rc, msg = _call(family=2, gen=0, T=4000, N=(1 << 24) - 1)
    assert rc == -1 and "pass a row cap" in msg, msg
    # a null or misaligned parameter is named; slots a family or a case does not have are not looked at
    rc, msg = _call(params=[0 if i == 30 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 8 of case 1 is null" in msg, msg
    rc, msg = _call(params=[0 if i == 70 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "shared parameter 4" in msg, msg
    rc, msg = _call(family=1, params=[0 if i == 30 else p for i, p in enumerate(ptrs)], T=4000, N=(1 << 24) - 1)
    assert rc == -1 and "pass a row cap" in msg, msg
    rc, msg = _call(family=1, params=[0 if i == 36 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 14 of case 1 is null" in msg, msg
    rc, msg = _call(family=2, params=[0 if i == 6 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 6 of case 0 is null" in msg, msg
    fam1 = [p if (i < 66 and (i % 22 < 6 or i % 22 >= 12)) else 0 for i, p in enumerate(ptrs)]
    fam2 = [p if (i < 66 and 6 <= i % 22 < 16) else 0 for i, p in enumerate(ptrs)]
    for family, tab in ((1, fam1), (2, fam2)):
        rc, msg = _call(family=family, params=tab, T=4000, N=(1 << 24) - 1)
        assert rc == -1 and "pass a row cap" in msg, (family, msg)
    rc, msg = _call(cases=2, params=[p if (22 <= i < 44 or i >= 66) else 0 for i, p in enumerate(ptrs)], T=4000, N=(1 << 24) - 1)
    assert rc == -1 and "pass a row cap" in msg, msg
    rc, msg = _call(params=[p + 4 if i == 17 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 17 of case 0 is misaligned" in msg, msg
    rc, msg = _call(params=[p + 2 if i == 2 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 2 of case 0 is misaligned" in msg, msg
    rc, msg = _call(x=0x1002)
    assert rc == -1 and "x must be 4-byte aligned" in msg, msg
    rc, msg = _call(ws=0x2004)
    assert rc == -1 and "workspace 16-byte aligned" in msg, msg
    rc, msg = _call(gen=0x91002)
    assert rc == -1 and "misaligned" in msg, msg
    rc, msg = _call(loss=1, y=0x3004)
    assert rc == -1 and "misaligned" in msg, msg
    rc, msg = _call(x=0x1004, y=0x3004, T=4000, N=(1 << 24) - 1)      # (x and float labels on 4 bytes are fine)
    assert rc == -1 and "pass a row cap" in msg, msg


def test_wide_sizes_are_refused_as_unsupported_without_a_device():
    """a hidden size above 128 in an LSTM the family runs: MFM_ERR_UNSUPPORTED with the size named; the same size in an LSTM the
    family does not have is not looked at"""
    wide_zy = [132 if i == 3 else v for i, v in enumerate(SIZES)]
    wide_zv = [132 if i == 2 else v for i, v in enumerate(SIZES)]
    wide_fl = [132 if i == 4 else v for i, v in enumerate(SIZES)]
    for family, sizes, refused in ((0, wide_zy, True), (2, wide_zy, True), (1, wide_zy, False), (0, wide_zv, True), (1, wide_zv, True),
                                   (2, wide_zv, False), (1, wide_fl, True), (2, wide_fl, False)):
        rc, msg = _call(family=family, sizes=sizes, T=4000, N=(1 << 24) - 1)
        if refused:
            assert rc == _lib.MFM_ERR_UNSUPPORTED and "132" in msg, (family, msg)
        else:
            assert rc == -1 and "pass a row cap" in msg, (family, msg)


def _model(name):
    from factorized_amd import mfm_model as M
    cfgs = configs.canonical_configs(dropout=False)
    return getattr(M, name)(*cfgs), cfgs


@pytest.mark.parametrize("name", CLASSES)
def test_predict_missing_on_a_cpu_model_raises(name):
    model, cfgs = _model(name)
    x = torch.zeros(3, 2, sum(cfgs[0]["input_dims"]))
    for missing in ("l", "each"):
        with pytest.raises(_lib.MfmError, match="move the model to the GPU"):
            model.predict_missing(x, missing=missing)
    with pytest.raises(ValueError, match="'l', 'a', 'v' or 'each'"):
        model.predict_missing(x, missing="x")
    with pytest.raises(ValueError, match="'l', 'a', 'v' or 'each'"):
        model.predict_missing(x, missing=0)
    if name != "seq2seq":
        with pytest.raises(ValueError, match="'l1' or 'ce'"):
            model.predict_missing(x, torch.zeros(2, 1), loss="mse")
    else:
        with pytest.raises(TypeError):
            model.predict_missing(x, torch.zeros(2, 1))               # (no label path: no labels)
    assert not [k for k in model.__dict__ if k.startswith("_missing")]      # (nothing was cached on the way to the refusal)


@pytest.mark.parametrize("name,family", zip(CLASSES, range(3)))
def test_sizes_and_parameter_tables(name, family):
    model, _ = _model(name)
    want = {0: SIZES, 1: [32, 8, 80, 1, 88, 8, 8, 1, 300, 5, 20, 1], 2: [1, 1, 1, 32, 1, 1, 1, 16, 300, 5, 20, 1]}[family]
    assert list(model._missing_sizes()) == want and model._MIS_FAMILY == family
    used = {0: lambda i: True, 1: lambda i: i < 66 and (i % 22 < 6 or i % 22 >= 12), 2: lambda i: i < 66 and 6 <= i % 22 < 16}[family]
    full = model._missing_params(("l", "a", "v"))
    assert len(full) == 74 and [p is not None for p in full] == [used(i) for i in range(74)]
    single = model._missing_params(("a",))
    assert len(single) == 74
    assert [p is not None for p in single] == [used(i) and (22 <= i < 44 or i >= 66) for i in range(74)]
    # the LSTM of a slot has the hidden size the size table names for it
    if family != 2:
        assert tuple(full[0].shape) == (4 * want[0], 5 + 20) and tuple(full[17].shape)[1] == (16 if family == 0 else 0) + want[4]
        assert tuple(full[12].shape) == (want[4], want[0])
    if family != 1:
        assert tuple(full[6].shape) == (4 * want[3], 5 + 20)
    if family == 2:
        assert tuple(full[12].shape) == (want[7], want[3]) and tuple(full[14].shape) == (want[11], want[7])


@pytest.mark.parametrize("name", CLASSES)
def test_the_module_pickles_and_keeps_its_state_dict_keys(name):
    from oracle import mfm_oracle_extra as X
    model, cfgs = _model(name)
    keys = list(model.state_dict().keys())
    assert keys == list(X.CLASSES[name](*cfgs).state_dict().keys())
    # a stubbed cache entry, as a call leaves it: a ctypes table cannot be pickled, so it has to be dropped
    model._missing_bufs = {(3, 2, 7, False, 1024, "cuda:0"): (torch.zeros(4), (C.c_void_p * 74)())}
    assert list(model.state_dict().keys()) == keys
    clone = pickle.loads(pickle.dumps(model))
    assert "_missing_bufs" not in clone.__dict__ and "_missing_bufs" in model.__dict__
    assert list(clone.state_dict().keys()) == keys
    for k, v in model.state_dict().items():
        assert torch.equal(v, clone.state_dict()[k]), k
